"""The three entry points of the sequence pipeline's MAVLink receive (include/aof_sequence_mavlink_rx.h, a section of aof.h):
the record's size and offsets as a C compiler lays the header out against the rig's ctypes record and the model's dtypes, the
exported symbols, which the package's surface does not carry, the header as C99 and C++11 in a translation unit that calls the
functions, and that the section refuses to be included alone and comes in behind aof_sequence_field.h.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import sequence_rx_ref as ref
import sequence_rx_rig as rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def test_records_have_the_headers_sizes_and_offsets(aof, tmp_path):
    args = ["sizeof(aof_seq_rx_params)", "offsetof(aof_seq_rx_params, n_bytes)", "offsetof(aof_seq_rx_params, max_samples)",
            "sizeof(aof_mavlink_rx_state)", "offsetof(aof_mavlink_rx_state, in_progress)", "sizeof(aof_imu_sample)"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "aof.h"\n'
           'int main(void) { printf("%s\\n", %s); return 0; }\n' % (" ".join(["%zu"] * len(args)), ", ".join(args)))
    f = tmp_path / "sizes.c"
    f.write_text(src)
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(f), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = rig.SeqRxParams
    assert got == [C.sizeof(P), P.n_bytes.offset, P.max_samples.offset, ref.STATE_DTYPE.itemsize, ref.STATE_DTYPE.fields["in_progress"][1],
                   ref.SAMPLE_DTYPE.itemsize] == [16, 0, 8, 128, 32, 24]
    assert ref.STATE_DTYPE == aof.MAVLINK_RX_STATE_DTYPE and ref.SAMPLE_DTYPE == aof.IMU_SAMPLE_DTYPE
    assert ref.IN_PROGRESS.itemsize == 96


def test_the_library_exports_the_three_calls_and_keeps_its_version(aof):
    lib = C.CDLL(aof.LIB_PATH)
    for name in rig.SYMBOLS:
        assert hasattr(lib, name), name
        assert name not in aof.EXPORTS, "the binding lives in tests/sequence_rx_rig.py, not in the package"
    rig.bind(aof)
    assert aof.lib.aof_version() == 102, "the feature adds entry points; the version stays"


def test_the_section_refuses_to_be_included_alone(tmp_path):
    f = tmp_path / "alone.c"
    f.write_text('#include <stdint.h>\n#include <stddef.h>\n#include "aof_sequence_mavlink_rx.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["cc", "-std=c99", "-fsyntax-only", "-I", INCLUDE, str(f)], capture_output=True, text=True)
    assert r.returncode != 0 and "aof_sequence_mavlink_rx.h is a section of it" in r.stderr, r.stderr
    hdr = open(os.path.join(INCLUDE, "aof.h")).read()
    assert hdr.count('#include "aof_sequence_mavlink_rx.h"') == 1
    assert hdr.index('#include "aof_sequence_field.h"') < hdr.index('#include "aof_sequence_mavlink_rx.h"') < hdr.index("---- measurement ----")
    assert "oracle" not in open(os.path.join(INCLUDE, "aof_sequence_mavlink_rx.h")).read().lower()


def test_header_is_valid_c99_and_cxx11(tmp_path):
    src = ('#include "aof.h"\n'
           'int use(aof_ctx *ctx, const uint8_t *bytes, const uint32_t *byte_end, aof_imu_sample *samples, uint32_t *sample_end,\n'
           '        aof_mavlink_rx_state *state, void *scratch) {\n'
           '    aof_seq_rx_params rp;\n'
           '    rp.n_bytes = 4096; rp.max_samples = 64;\n'
           '    if (aof_sequence_mavlink_rx_host(&rp, 4, bytes, byte_end, samples, sample_end, state)) return 1;\n'
           '    if (aof_sequence_mavlink_rx_scratch_bytes(rp.n_bytes) == 0) return 2;\n'
           '    return aof_sequence_mavlink_rx_device(ctx, &rp, 4, bytes, byte_end, samples, sample_end, state, scratch,\n'
           '                                          aof_sequence_mavlink_rx_scratch_bytes(rp.n_bytes), 0) + (int)sizeof(*state);\n'
           '}\n')
    for cc, name, std in (("cc", "t.c", "-std=c99"), ("g++", "t.cpp", "-std=c++11")):
        assert shutil.which(cc), cc
        f = tmp_path / name
        f.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, str(f)], check=True)
