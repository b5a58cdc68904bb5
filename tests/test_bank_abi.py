"""The host-only side of the stream bank (include/aof.h, "a bank of live streams"): the layout of a bank, the record
and parameter structs, and what aof_bank_layout / aof_set_bank_path refuse -- no device needed."""
import ctypes as C

import numpy as np
import pytest

EINVAL = -22


def layout(aof, p, **kw):
    return aof.bank_layout(p, aof.bank_params(**kw))


def test_record_and_parameter_structs_match_the_header(aof):
    assert aof.TICK_DTYPE.itemsize == 48                                   # sizeof(aof_tick_record)
    assert aof.TICK_DTYPE.fields["pixel"][1] == 32 and aof.TICK_DTYPE.fields["frame"][1] == 28
    assert aof.TICK_DTYPE.fields["pixel"][0] == aof.FLOW_DTYPE
    assert (aof.TICK_HELD, aof.TICK_IDLE) == (-1, -2)
    assert C.sizeof(aof.BankParams) == 48                                  # i32, pad, i64, 2 f32, i32, pad, u64, 3 u8, pad
    assert aof.BankParams.frame_stride.offset == 8 and aof.BankParams.offset_timestamp_usec.offset == 32
    assert C.sizeof(aof.BankLayout) == 4 * C.sizeof(C.c_size_t)
    assert aof.BANK_STATE_BYTES == 64


@pytest.mark.parametrize("size,kw", [((64, 64), {}), ((128, 128), dict(pyramid_levels=2, mean_subtract=1)),
                                     ((192, 160), None), ((160, 128), dict(tile=16, search=8))])
def test_bank_layout_regions(aof, size, kw):
    w, h = size
    p = aof.default_params(w, h, subpixel=1) if kw is None else (
        aof.px4flow_params(w, h, **kw) if "tile" not in kw else aof.default_params(w, h, **kw))
    last = 0
    for S in (1, 2, 24, 300, 4096):
        for stride in (0, w * h, w * h + 16, 2 * w * h):
            L = layout(aof, p, n_streams=S, frame_stride=stride)
            offs = [L.frames, L.state, L.scratch, L.total_bytes]
            assert offs == sorted(offs) and all(o % 256 == 0 for o in offs), (S, stride, offs)
            assert L.state - L.frames >= S * (stride or w * h)
            assert L.scratch - L.state >= S * aof.BANK_STATE_BYTES
            # the flow engine's workspace for S pairs, and the tick's aof_flow [S] behind it
            assert L.total_bytes - L.scratch >= aof.workspace_layout(p, S).total_bytes + 16 * S
        total = layout(aof, p, n_streams=S).total_bytes
        assert total > last, "the bank grows with the number of streams"
        last = total


def test_bank_layout_refuses_bad_arguments(aof):
    p = aof.px4flow_params(64, 64)
    ok = dict(n_streams=4)
    call = aof.lib.aof_bank_layout
    L = aof.BankLayout()
    assert call(C.byref(p), C.byref(aof.bank_params(**ok)), C.byref(L)) == 0
    assert call(None, C.byref(aof.bank_params(**ok)), C.byref(L)) == EINVAL
    assert call(C.byref(p), None, C.byref(L)) == EINVAL
    assert call(C.byref(p), C.byref(aof.bank_params(**ok)), None) == EINVAL
    for bad in (dict(n_streams=0), dict(n_streams=-3), dict(n_streams=4, frame_stride=64 * 64 - 16),
                dict(n_streams=4, frame_stride=64 * 64 + 8), dict(n_streams=4, frame_stride=-4096),
                dict(n_streams=4, focal_x=0.0), dict(n_streams=4, focal_y=-1.0), dict(n_streams=4, focal_x=float("nan"))):
        assert call(C.byref(p), C.byref(aof.bank_params(**bad)), C.byref(L)) == EINVAL, bad
        with pytest.raises(aof.AofError):
            aof.bank_layout(p, aof.bank_params(**bad))
    broken = aof.px4flow_params(64, 64, tile=12)                           # parameters aof_params_check refuses
    assert call(C.byref(broken), C.byref(aof.bank_params(**ok)), C.byref(L)) == EINVAL


def test_bank_entry_points_refuse_a_null_context(aof):
    """No device needed: every entry point checks the context first."""
    for path in (0, 1, 2, 3, -1):
        assert aof.lib.aof_set_bank_path(None, path) == EINVAL
    bp = aof.bank_params(n_streams=2)
    buf = np.zeros(1 << 16, np.uint8)
    assert aof.lib.aof_bank_reset_device(None, C.byref(bp), None, buf.ctypes.data, buf.size, None) == EINVAL
    assert aof.lib.aof_bank_push_device(None, C.byref(bp), buf.ctypes.data, buf.ctypes.data, None, None, buf.ctypes.data,
                                        buf.size, buf.ctypes.data, None, None, None) == EINVAL


def test_header_declares_the_bank(aof):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "aof.h")).read()
    for name in ("aof_bank_layout", "aof_bank_reset_device", "aof_bank_push_device", "aof_set_bank_path"):
        assert re.search(r"\bint " + name + r"\(", text), name
        assert name in aof.EXPORTS
    assert "#define AOF_VERSION 102" in text


def test_header_is_valid_c_and_cxx(tmp_path):
    """The bank's layout struct and the function that fills it share a name: the struct is a tag only, so that the
    header stays plain C (one name space for typedefs and functions) as well as C++."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ('#include "aof.h"\n'
           'int use(const aof_params *p, const aof_bank_params *bp) { struct aof_bank_layout L; aof_tick_record r; '
           '(void)r; return aof_bank_layout(p, bp, &L) + (int)sizeof(r); }\n')
    for cc, name, std in (("cc", "t.c", "-std=c99"), ("g++", "t.cpp", "-std=c++11")):   # (the compilers build() uses)
        assert shutil.which(cc), cc
        f = tmp_path / name
        f.write_text(src)
        subprocess.run([cc, std, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(root, "include"), str(f)], check=True)
