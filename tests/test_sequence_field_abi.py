"""The two entry points of the sequence pipeline's motion field (include/aof_sequence_field.h, a section of aof.h) and the
records they share with the stream bank's: sizes and offsets as a C compiler lays the header out against the rig's and the
model's dtypes, the exported symbols, the header as C99 and C++11, and that the section refuses to be included alone.  CPU
only."""
import ctypes as C
import os
import shutil
import subprocess

import sequence_field_ref as ref
import sequence_field_rig as rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
STRUCTS = (("aof_bank_field_record", rig.RECORD_DTYPE), ("aof_bank_field_state", rig.STATE_DTYPE), ("aof_seq_record", ref.SEQ_RECORD_DTYPE))


def test_records_have_the_headers_sizes_and_offsets(aof, tmp_path):
    fmt, args, want = [], [], []
    for struct, dtype in STRUCTS:
        args.append(f"sizeof({struct})")
        want.append(dtype.itemsize)
        for f in dtype.names:
            args.append(f"offsetof({struct}, {f})")
            want.append(dtype.fields[f][1])
    fmt = " ".join(["%zu"] * len(args))
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "aof.h"\n'
           'int main(void) { printf("%s\\n", %s); return 0; }\n' % (fmt, ", ".join(args)))
    f = tmp_path / "sizes.c"
    f.write_text(src)
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(f), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert got[0] == 48 and got[13] == 64 and got[-9] == 32
    assert ref.SEQ_RECORD_DTYPE == aof.SEQ_RECORD_DTYPE, "the model restates the record on its own"


def test_the_library_exports_the_two_calls_and_keeps_its_version(aof):
    lib = C.CDLL(aof.LIB_PATH)
    for name in rig.SYMBOLS:
        assert hasattr(lib, name), name
        assert name not in aof.EXPORTS, "the binding lives in tests/sequence_field_rig.py, not in the package"
    rig.bind(aof)
    assert aof.lib.aof_version() == 102, "the feature adds entry points; the version stays"


def test_the_section_refuses_to_be_included_alone(tmp_path):
    f = tmp_path / "alone.c"
    f.write_text('#include <stdint.h>\n#include <stddef.h>\n#include "aof_sequence_field.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["cc", "-std=c99", "-fsyntax-only", "-I", INCLUDE, str(f)], capture_output=True, text=True)
    assert r.returncode != 0 and "aof_sequence_field.h is a section of it" in r.stderr, r.stderr
    hdr = open(os.path.join(INCLUDE, "aof.h")).read()
    assert '#include "aof_sequence_field.h"' in hdr
    assert hdr.index('#include "aof_sequence_imu.h"') < hdr.index('#include "aof_sequence_field.h"')
    assert "oracle" not in open(os.path.join(INCLUDE, "aof_sequence_field.h")).read().lower()


def test_header_is_valid_c99_and_cxx11(tmp_path):
    src = ('#include "aof.h"\n'
           'int use(aof_ctx *ctx, const aof_params *p, const aof_sequence_params *sp, const aof_block *b, const uint8_t *sd,\n'
           '        const aof_flow *fl, const aof_seq_record *r, aof_field *f, aof_bank_field_record *o, aof_bank_field_state *s, void *ws) {\n'
           '    aof_field_params fp;\n'
           '    if (aof_field_params_default(&fp)) return 1;\n'
           '    if (aof_sequence_field_host(p, sp, &fp, 4, b, sd, fl, r, 2u, f, o, s)) return 2;\n'
           '    if (o->status == AOF_TICK_HELD) return 3;\n'
           '    return aof_sequence_field_device(ctx, sp, &fp, 4, ws, 4096, f, o, s, 0) + (int)sizeof(*s);\n'
           '}\n')
    for cc, name, std in (("cc", "t.c", "-std=c99"), ("g++", "t.cpp", "-std=c++11")):
        assert shutil.which(cc), cc
        f = tmp_path / name
        f.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, str(f)], check=True)


def test_the_device_call_without_a_context_is_refused_first(aof):
    """No context can exist without a device: the context check comes first and answers -EINVAL whatever else is passed."""
    call = rig.bind(aof).aof_sequence_field_device
    assert call(None, None, None, 4, None, 0, None, None, None, None) == rig.EINVAL
    sp, fp = aof.sequence_params(64, 64, 64, 64), aof.field_params()
    assert call(None, C.byref(sp), C.byref(fp), 4, None, 0, None, None, None, None) == rig.EINVAL
