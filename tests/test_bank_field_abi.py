"""The structures and entry points of the stream bank's motion field (include/aof.h): sizes and offsets as a C compiler lays
the header out against the rig's dtypes (tests/bank_field_rig.py, where the records are written once), the three symbols in
libaof.so and the three shims in the facade library, the version, and the header as C99 and C++11.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import bank_field_rig as rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STATE_FIELDS = ("sum_zoom", "sum_rotation", "sum_centre_x", "sum_centre_y", "pairs", "fits", "used", "published", "reserved")
RECORD_FIELDS = ("status", "dt_us", "zoom", "rotation", "centre_x", "centre_y", "flow_x", "flow_y", "pairs", "fits", "used", "frame")


def test_structs_have_the_headers_sizes_and_offsets(tmp_path):
    fmt, args = [], []
    for struct, fields in (("aof_bank_field_state", STATE_FIELDS), ("aof_bank_field_record", RECORD_FIELDS)):
        fmt += ["%zu", "%zu"]
        args += [f"sizeof({struct})", f"_Alignof({struct})"]
        for f in fields:
            fmt.append("%zu")
            args.append(f"offsetof({struct}, {f})")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "aof.h"\n'
           'int main(void) { printf("%s %%d %%d %%d %%d %%d %%d\\n", %s, AOF_TICK_HELD, AOF_TICK_IDLE, AOF_TICK_STALE_GYRO, AOF_TICK_NO_OFFSET, '
           'AOF_TICK_BAD_SENSOR, AOF_VERSION); return 0; }\n' % (" ".join(fmt), ", ".join(args)))
    f = tmp_path / "sizes.c"
    f.write_text(src)
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for dtype, fields, align in ((rig.STATE_DTYPE, STATE_FIELDS, 8), (rig.RECORD_DTYPE, RECORD_FIELDS, 4)):
        assert dtype.names == fields
        want += [dtype.itemsize, align] + [dtype.fields[n][1] for n in fields]
    want += [rig.HELD, rig.IDLE, rig.STALE_GYRO, rig.NO_OFFSET, rig.BAD_SENSOR, 102]
    assert got == want
    assert got[:11] == [64, 8, 0, 8, 16, 24, 32, 36, 40, 44, 48] and got[11:25] == [48, 4] + list(range(0, 48, 4))
    assert rig.STATE_DTYPE["reserved"].itemsize == 16


def test_the_symbols_exist_and_the_version_stays(aof):
    lib = rig.bind(aof)
    for name in rig.SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.aof_version() == 102, "the feature adds entry points; the version stays"
    # the package's own surface does not move: the rig carries the binding
    assert not set(rig.SYMBOLS) & set(aof.EXPORTS)
    f = rig.facade(aof)
    for name in rig.FACADE_SYMBOLS:
        assert hasattr(f, name), name
    plain = C.CDLL(aof.LIB_PATH)
    assert all(hasattr(plain, name) for name in rig.SYMBOLS)


def test_header_is_valid_c99_and_cxx11(tmp_path):
    src = ('#include "aof.h"\n'
           'int use(aof_ctx *ctx, const aof_params *p, const aof_bank_params *bp, const aof_tick_record *r, aof_bank_field_state *s,\n'
           '        aof_field *f, aof_bank_field_record *o, const aof_block *b, const void *bank) {\n'
           '    aof_field_params fp;\n'
           '    if (aof_field_params_default(&fp)) return 1;\n'
           '    if (aof_bank_field_host(p, bp, 0, &fp, b, 0, r, s, f, o)) return 2;\n'
           '    if (o->status == AOF_TICK_HELD || o->status == AOF_TICK_BAD_SENSOR) return 3;\n'
           '    if (aof_bank_field_reset_device(ctx, 1, 0, s, 0)) return 4;\n'
           '    return aof_bank_field_device(ctx, bp, &fp, bank, 4096, r, s, f, o, 0) + (int)sizeof(*s) + (int)sizeof(s->reserved);\n'
           '}\n')
    for cc, name, std in (("cc", "t.c", "-std=c99"), ("g++", "t.cpp", "-std=c++11")):
        assert shutil.which(cc), cc
        f = tmp_path / name
        f.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(f)], check=True)
