"""The structures and entry points of the stream bank's auto-exposure control (include/aof.h): sizes and offsets as a C
compiler lays the header out, the binding's dtypes, what is refused without a device, and the header as C99 and C++11.
CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import exposure_control_ref as xref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22

STATE_FIELDS = ("msv_error_old", "msv_error_int", "exposure", "gain", "reserved", "updates")
COMMAND_FIELDS = ("exposure", "gain", "flags", "msv_error", "msv_error_int", "update")
CONTROL_FIELDS = ("msv_target", "exposure_p", "exposure_i", "exposure_d", "gain_p", "gain_i", "gain_d",
                  "exposure_change_threshold", "exposure_max", "gain_change_threshold", "gain_max")


def test_structs_have_the_headers_sizes_and_offsets(aof, tmp_path):
    fmt, args = [], []
    for struct, fields in (("aof_exposure_state", STATE_FIELDS), ("aof_exposure_command", COMMAND_FIELDS),
                           ("aof_exposure_control", CONTROL_FIELDS)):
        fmt.append("%zu")
        args.append(f"sizeof({struct})")
        for f in fields:
            fmt.append("%zu")
            args.append(f"offsetof({struct}, {f})")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "aof.h"\n'
           'int main(void) { printf("%s %%u %%u %%u\\n", %s, AOF_EXPOSURE_UPDATED, AOF_EXPOSURE_SET_EXPOSURE, AOF_EXPOSURE_SET_GAIN); '
           'return 0; }\n' % (" ".join(fmt), ", ".join(args)))
    f = tmp_path / "sizes.c"
    f.write_text(src)
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for dtype, fields in ((aof.EXPOSURE_STATE_DTYPE, STATE_FIELDS), (aof.EXPOSURE_COMMAND_DTYPE, COMMAND_FIELDS)):
        assert dtype.names == fields
        want += [dtype.itemsize] + [dtype.fields[n][1] for n in fields]
    assert tuple(n for n, _ in aof.ExposureControl._fields_) == CONTROL_FIELDS
    want += [C.sizeof(aof.ExposureControl)] + [getattr(aof.ExposureControl, n).offset for n in CONTROL_FIELDS]
    want += [aof.EXPOSURE_UPDATED, aof.EXPOSURE_SET_EXPOSURE, aof.EXPOSURE_SET_GAIN]
    assert got == want
    assert got[:7] == [16, 0, 4, 8, 10, 11, 12] and got[7:14] == [16, 0, 2, 3, 4, 8, 12] and got[14] == 44 and got[-3:] == [1, 2, 4]
    # the model restates the layouts on its own
    assert aof.EXPOSURE_STATE_DTYPE == xref.STATE_DTYPE and aof.EXPOSURE_COMMAND_DTYPE == xref.COMMAND_DTYPE
    assert aof.EXPOSURE_DTYPE == xref.RECORD_DTYPE
    assert (xref.UPDATED, xref.SET_EXPOSURE, xref.SET_GAIN) == (1, 2, 4)


def test_the_binding_exposes_the_feature(aof):
    for name in ("aof_exposure_control_default", "aof_bank_exposure_reset_device", "aof_bank_exposure_control_device",
                 "aof_exposure_control_host"):
        assert name in aof.EXPORTS and hasattr(aof.lib, name)
    assert callable(aof.FlowEngine.bank_exposure_reset) and callable(aof.FlowEngine.bank_exposure_control)
    assert callable(aof.exposure_control_host) and callable(aof.exposure_control_default)
    for name in ("enableCamera", "pushCamera", "exposureCommands"):
        assert callable(getattr(aof.OpticalFlowBank, name))
    assert aof.lib.aof_version() == 102, "the feature adds entry points; the version stays"


def test_calls_without_a_context_are_refused_first(aof):
    """No context can exist without a device: the context check comes first and answers -EINVAL whatever else is passed."""
    ec = aof.exposure_control_default()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    control, reset = aof.lib.aof_bank_exposure_control_device, aof.lib.aof_bank_exposure_reset_device
    assert control(None, C.byref(ec), 1, 1, p, p, p, None) == EINVAL
    assert control(None, None, 0, 99, None, None, None, None) == EINVAL
    assert reset(None, 1, None, 1, 1, None, None, p, None) == EINVAL
    assert reset(None, 0, None, 0, 0, None, None, None, None) == EINVAL
    assert not buf.any()


def test_header_is_valid_c99_and_cxx11(tmp_path):
    src = ('#include "aof.h"\n'
           'int use(aof_ctx *ctx, const aof_exposure_record *r, aof_exposure_state *s, aof_exposure_command *c) {\n'
           '    aof_exposure_control ec;\n'
           '    if (aof_exposure_control_default(&ec)) return 1;\n'
           '    if (aof_exposure_control_host(&ec, 1, 1, r, s, c)) return 2;\n'
           '    if (c->flags & AOF_EXPOSURE_SET_GAIN) return 3;\n'
           '    if (aof_bank_exposure_reset_device(ctx, 1, 0, 1, 1, 0, 0, s, 0)) return 4;\n'
           '    return aof_bank_exposure_control_device(ctx, &ec, 1, AOF_BANK_BURST_MAX, r, s, c, 0) + (int)sizeof(*s);\n'
           '}\n')
    for cc, name, std in (("cc", "t.c", "-std=c99"), ("g++", "t.cpp", "-std=c++11")):
        assert shutil.which(cc), cc
        f = tmp_path / name
        f.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(f)], check=True)
