"""The record and the two entry points of the sequence pipeline's IMU call (include/aof_sequence_imu.h, a section of aof.h):
sizes and offsets as a C compiler lays the header out against the rig's ctypes record and the model's dtypes, the exported
symbols, the header as C99 and C++11, and that the section refuses to be included alone.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import sequence_imu_ref as ref
import sequence_imu_rig as rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PARAM_FIELDS = ("n_samples", "offset0", "system_id", "component_id", "first_seq")
RECORD_FIELDS = ("frame", "quality", "dt_us", "flow_x", "flow_y", "gyro_x", "gyro_y", "gyro_z")


def test_records_have_the_headers_sizes_and_offsets(aof, tmp_path):
    fmt, args = [], []
    for struct, fields in (("aof_seq_imu_params", PARAM_FIELDS), ("aof_seq_record", RECORD_FIELDS)):
        fmt.append("%zu")
        args.append(f"sizeof({struct})")
        for f in fields:
            fmt.append("%zu")
            args.append(f"offsetof({struct}, {f})")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "aof.h"\n'
           'int main(void) { printf("%s\\n", %s); return 0; }\n' % (" ".join(fmt), ", ".join(args)))
    f = tmp_path / "sizes.c"
    f.write_text(src)
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(f), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert tuple(n for n, _ in rig.SeqImuParams._fields_) == PARAM_FIELDS
    want = [C.sizeof(rig.SeqImuParams)] + [getattr(rig.SeqImuParams, n).offset for n in PARAM_FIELDS]
    want += [ref.RECORD_DTYPE.itemsize] + [ref.RECORD_DTYPE.fields[n][1] for n in RECORD_FIELDS]
    assert got == want
    assert got[:6] == [24, 0, 8, 16, 17, 18] and got[6:] == [32, 0, 4, 8, 12, 16, 20, 24, 28]
    assert ref.RECORD_DTYPE == aof.SEQ_RECORD_DTYPE, "the model restates the record on its own"
    assert ref.SAMPLE_DTYPE == aof.IMU_SAMPLE_DTYPE and ref.STATE_DTYPE == aof.IMU_STATE_DTYPE


def test_the_library_exports_the_two_calls_and_keeps_its_version(aof):
    lib = C.CDLL(aof.LIB_PATH)
    for name in rig.SYMBOLS:
        assert hasattr(lib, name), name
        assert name not in aof.EXPORTS, "the binding lives in tests/sequence_imu_rig.py, not in the package"
    rig.bind(aof)
    assert aof.lib.aof_version() == 102, "the feature adds entry points; the version stays"


def test_the_section_refuses_to_be_included_alone(tmp_path):
    f = tmp_path / "alone.c"
    f.write_text('#include <stdint.h>\n#include <stddef.h>\n#include "aof_sequence_imu.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["cc", "-std=c99", "-fsyntax-only", "-I", INCLUDE, str(f)], capture_output=True, text=True)
    assert r.returncode != 0 and "aof_sequence_imu.h is a section of it" in r.stderr, r.stderr
    hdr = open(os.path.join(INCLUDE, "aof.h")).read()
    assert '#include "aof_sequence_imu.h"' in hdr
    assert "oracle" not in open(os.path.join(INCLUDE, "aof_sequence_imu.h")).read().lower()


def test_header_is_valid_c99_and_cxx11(tmp_path):
    src = ('#include "aof.h"\n'
           'int use(aof_ctx *ctx, const aof_sequence_params *sp, const uint64_t *t, const aof_imu_sample *m, const uint32_t *e,\n'
           '        aof_seq_record *r, uint32_t *count, unsigned char *f, unsigned char *l, aof_imu_state *s, void *ws) {\n'
           '    aof_seq_imu_params ip = {250, 0, 1, 100, 0};\n'
           '    if (aof_sequence_imu_host(&ip, 4, t, m, e, r, count, f, l, s)) return 1;\n'
           '    if (r->quality == AOF_TICK_STALE_GYRO || r->quality == AOF_TICK_NO_OFFSET) return 2;\n'
           '    return aof_sequence_imu_device(ctx, sp, &ip, 4, t, m, e, ws, 4096, s, 0) + (int)sizeof(ip);\n'
           '}\n')
    for cc, name, std in (("cc", "t.c", "-std=c99"), ("g++", "t.cpp", "-std=c++11")):
        assert shutil.which(cc), cc
        f = tmp_path / name
        f.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, str(f)], check=True)


def test_the_device_call_without_a_context_is_refused_first(aof):
    """No context can exist without a device: the context check comes first and answers -EINVAL whatever else is passed."""
    call = rig.bind(aof).aof_sequence_imu_device
    assert call(None, None, None, 4, None, None, None, None, 0, None, None) == rig.EINVAL
    sp, ip = aof.sequence_params(64, 64, 64, 64), rig.params(0)
    assert call(None, C.byref(sp), C.byref(ip), 4, None, None, None, None, 0, None, None) == rig.EINVAL
