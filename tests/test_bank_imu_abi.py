"""The structures and entry points of the stream bank's IMU (include/aof.h): sizes and offsets as a C compiler lays the
header out, the binding's dtypes, every refusal -- each returns its code and writes nothing, on the host function and,
where no device is needed, on the device entries' argument checks -- and the header as C99 and C++11.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import imu_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22

SAMPLE_FIELDS = ("time_usec", "xgyro", "ygyro", "zgyro", "reserved")
STATE_FIELDS = ("gyro_x", "gyro_y", "gyro_z", "prev_time_usec", "last_taken_time_usec", "offset_timestamp_usec", "messages",
                "samples_integrated", "samples_rejected", "dropped")
PARAM_FIELDS = ("n_streams", "n_rounds", "max_samples", "system_id", "component_id", "first_seq")


def test_structs_have_the_headers_sizes_and_offsets(aof, tmp_path):
    fmt, args = [], []
    for struct, fields in (("aof_imu_sample", SAMPLE_FIELDS), ("aof_imu_state", STATE_FIELDS), ("aof_imu_params", PARAM_FIELDS)):
        fmt.append("%zu")
        args.append(f"sizeof({struct})")
        for f in fields:
            fmt.append("%zu")
            args.append(f"offsetof({struct}, {f})")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "aof.h"\n'
           'int main(void) { printf("%s %%d %%d %%d\\n", %s, AOF_IMU_SLOTS_MAX, AOF_TICK_STALE_GYRO, AOF_TICK_NO_OFFSET); '
           'return 0; }\n' % (" ".join(fmt), ", ".join(args)))
    f = tmp_path / "sizes.c"
    f.write_text(src)
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for dtype, fields in ((aof.IMU_SAMPLE_DTYPE, SAMPLE_FIELDS), (aof.IMU_STATE_DTYPE, STATE_FIELDS)):
        assert dtype.names == fields
        want += [dtype.itemsize] + [dtype.fields[n][1] for n in fields]
    assert tuple(n for n, _ in aof.ImuParams._fields_) == PARAM_FIELDS
    want += [C.sizeof(aof.ImuParams)] + [getattr(aof.ImuParams, n).offset for n in PARAM_FIELDS]
    want += [aof.IMU_SLOTS_MAX, aof.TICK_STALE_GYRO, aof.TICK_NO_OFFSET]
    assert got == want
    assert got[:6] == [24, 0, 8, 12, 16, 20]
    assert got[6:17] == [64, 0, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    assert got[17:24] == [16, 0, 4, 8, 12, 13, 14] and got[-3:] == [16, -3, -4]
    # the model restates the layouts on its own
    assert aof.IMU_SAMPLE_DTYPE == ref.SAMPLE_DTYPE and aof.IMU_STATE_DTYPE == ref.STATE_DTYPE


def test_the_binding_exposes_the_feature(aof):
    for name in ("aof_bank_imu_reset_device", "aof_bank_imu_device", "aof_bank_imu_host"):
        assert name in aof.EXPORTS and hasattr(aof.lib, name)
    assert callable(aof.FlowEngine.bank_imu_reset) and callable(aof.FlowEngine.bank_imu) and callable(aof.bank_imu_host)
    for name in ("enableImu", "pushImu"):
        assert callable(getattr(aof.OpticalFlowBank, name))
    assert aof.lib.aof_version() == 102, "the feature adds entry points; the version stays"


def test_the_header_section_does_not_name_the_checker():
    hdr = open(os.path.join(ROOT, "include", "aof.h")).read()
    assert "oracle" not in hdr.lower()


class Call:
    """One valid call of aof_bank_imu_host on sentinel-filled memory; refused() changes one argument and checks the
    code and that not one byte was written."""

    def __init__(self, aof):
        self.aof = aof
        K, M, S = 2, 3, 5
        f = ref.random_family(seed=1, S=S, K=K, M=M)
        self.ip = aof.imu_params(S, K, M)
        # every buffer inside one 8-byte aligned block, so that a misaligned pointer still points into owned memory
        self.buf = {n: np.zeros(size + 16, np.uint64) for n, size in
                    (("samples", K * M * S * 3), ("counts", K * S), ("times", K * S), ("records", K * S * 6), ("states", S * 8),
                     ("out", K * S * 6), ("frames", K * S * 7), ("lengths", K * S))}
        self.buf["samples"][:K * M * S * 3] = f["samples"].view(np.uint64).ravel()
        self.buf["times"][:K * S] = f["times"].ravel()
        self.buf["records"][:K * S * 6] = f["records"].view(np.uint64).ravel()
        for n in ("states", "out", "frames", "lengths"):
            self.buf[n][:] = 0xA5A5A5A5A5A5A5A5
        self.written = ("states", "out", "frames", "lengths")

    def args(self, **change):
        a = dict(ip=C.byref(self.ip), **{n: b.ctypes.data for n, b in self.buf.items()})
        a.update(change)
        return [a[n] for n in ("ip", "samples", "counts", "times", "records", "states", "out", "frames", "lengths")]

    def host(self, **change):
        before = {n: self.buf[n].copy() for n in self.written}
        rc = self.aof.lib.aof_bank_imu_host(*self.args(**change))
        return rc, all((self.buf[n] == before[n]).all() for n in self.written)


def test_the_valid_call_is_accepted(aof):
    c = Call(aof)
    rc, untouched = c.host()
    assert rc == 0 and not untouched
    c = Call(aof)
    assert c.host(out=c.buf["records"].ctypes.data)[0] == 0, "in place"
    c = Call(aof)
    assert c.host(frames=None, lengths=None)[0] == 0 and c.host(counts=None)[0] == 0


REFUSALS = {
    "null params": dict(ip=None),
    "null samples": dict(samples=None),
    "null times": dict(times=None),
    "null records in": dict(records=None),
    "null records out": dict(out=None),
    "null state": dict(states=None),
    "frames without lengths": dict(lengths=None),
    "lengths without frames": dict(frames=None),
    "n_streams 0": dict(n_streams=0),
    "n_streams negative": dict(n_streams=-3),
    "n_rounds 0": dict(n_rounds=0),
    "n_rounds above the maximum": dict(n_rounds=17),
    "max_samples 0": dict(max_samples=0),
    "max_samples above the maximum": dict(max_samples=17),
    "samples at 4 mod 8": dict(samples=+4),
    "states at 4 mod 8": dict(states=+4),
    "times at 4 mod 8": dict(times=+4),
    "records in at 2 mod 4": dict(records=+2),
    "records out at 2 mod 4": dict(out=+2),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_the_host_function_refuses_and_writes_nothing(aof, name):
    c = Call(aof)
    change = {}
    for key, v in REFUSALS[name].items():
        if key in ("n_streams", "n_rounds", "max_samples"):
            setattr(c.ip, key, v)
        elif v is None:
            change[key] = None
        else:
            change[key] = c.buf[key].ctypes.data + v
    rc, untouched = c.host(**change)
    assert rc == EINVAL and untouched


def test_records_need_four_byte_alignment_only(aof):
    c = Call(aof)
    shifted = c.buf["records"].view(np.uint8)
    shifted[4:4 + 2 * 5 * 48] = shifted[:2 * 5 * 48].copy()
    assert c.host(records=c.buf["records"].ctypes.data + 4, out=c.buf["out"].ctypes.data + 4)[0] == 0


def test_device_calls_without_a_context_are_refused_first(aof):
    """No context can exist without a device: the context check comes first and answers -EINVAL whatever else is passed."""
    c = Call(aof)
    before = {n: c.buf[n].copy() for n in c.written}
    device, reset = aof.lib.aof_bank_imu_device, aof.lib.aof_bank_imu_reset_device
    assert device(None, *c.args(), None) == EINVAL
    assert device(None, None, None, None, None, None, None, None, None, None, None) == EINVAL
    assert reset(None, 5, None, 0, c.buf["states"].ctypes.data, None) == EINVAL
    assert reset(None, 0, None, 7, None, None) == EINVAL
    assert all((c.buf[n] == before[n]).all() for n in c.written)


def test_header_is_valid_c99_and_cxx11(tmp_path):
    src = ('#include "aof.h"\n'
           'int use(aof_ctx *ctx, const aof_imu_sample *m, const unsigned char *n, const uint64_t *t, aof_tick_record *r,\n'
           '        aof_imu_state *s, unsigned char *f, unsigned char *l) {\n'
           '    aof_imu_params ip = {1, AOF_BANK_BURST_MAX, AOF_IMU_SLOTS_MAX, 1, 100, 0};\n'
           '    if (aof_bank_imu_host(&ip, m, n, t, r, s, r, f, l)) return 1;\n'
           '    if (r->quality == AOF_TICK_STALE_GYRO || r->quality == AOF_TICK_NO_OFFSET) return 2;\n'
           '    if (aof_bank_imu_reset_device(ctx, 1, 0, 0, s, 0)) return 3;\n'
           '    return aof_bank_imu_device(ctx, &ip, m, n, t, r, s, r, f, l, 0) + (int)sizeof(*s) + (int)sizeof(*m);\n'
           '}\n')
    for cc, name, std in (("cc", "t.c", "-std=c99"), ("g++", "t.cpp", "-std=c++11")):
        assert shutil.which(cc), cc
        f = tmp_path / name
        f.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(f)], check=True)
