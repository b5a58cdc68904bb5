"""The host-only side of the stream bank's bursts (include/aof.h, "the stream bank in bursts"): the two entry points
exist in the library, the header and the binding, the parameter struct has the header's layout, and a call without a
context is refused before anything else is looked at (the only refusal a machine without a device can reach)."""
import ctypes as C
import os
import re

import numpy as np

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aof_bank_push_burst_device", "aof_bank_push_camera_burst_device")


def test_library_header_and_binding_have_both_entry_points(aof):
    text = open(os.path.join(ROOT, "include", "aof.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", text), name
        assert name in aof.EXPORTS
        assert getattr(aof.lib, name).restype is C.c_int
    assert re.search(r"#define AOF_BANK_BURST_MAX 16\b", text) and aof.BANK_BURST_MAX == 16
    assert "#define AOF_VERSION 102" in text
    assert callable(aof.FlowEngine.bank_push_burst) and callable(aof.FlowEngine.bank_push_camera_burst)


def test_structs_have_the_headers_sizes(aof, tmp_path):
    """sizeof and offsets as the C compiler lays the header's structs out."""
    import subprocess
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "aof.h"\n'
           'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(aof_bank_burst), offsetof(aof_bank_burst, n_rounds), '
           'offsetof(aof_bank_burst, round_stride), sizeof(aof_bank_params), sizeof(aof_bank_camera), sizeof(aof_tick_record)); return 0; }\n')
    f = tmp_path / "sizes.c"
    f.write_text(src)
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(aof.BankBurst), aof.BankBurst.n_rounds.offset, aof.BankBurst.round_stride.offset,
                   C.sizeof(aof.BankParams), C.sizeof(aof.BankCamera), aof.TICK_DTYPE.itemsize]
    assert got[:3] == [16, 0, 8]
    b = aof.bank_burst_params(5, 4096 * 3)
    assert (b.n_rounds, b.round_stride) == (5, 12288) and aof.bank_burst_params(7).round_stride == 0


def test_a_call_without_a_context_is_refused_first_whatever_else_is_wrong(aof):
    """No context can exist without a device, so this proves one thing only: the context check comes first, and a call
    without one answers -EINVAL and touches nothing, whatever the other arguments are (NULL parameters or burst,
    n_rounds 0 or 17, a round_stride below one round or off the 16-byte grid).  The burst's own checks (check_burst) are
    not reached here; tests/test_gpu_bank_burst.py::test_burst_entry_points_argument_handling covers them on a device."""
    bp = aof.bank_params(n_streams=2)
    cam = aof.bank_camera_params(320, 240, 64, 64)
    buf = np.full(1 << 16, 0xEE, np.uint8)
    d = buf.ctypes.data
    plain, camera = (getattr(aof.lib, n) for n in NAMES)
    B = aof.bank_burst_params
    bursts = [B(5), None, B(0), B(17), B(5, 2 * 4096 - 16), B(5, 2 * 4096 + 8), B(5, 2 * 320 * 240 - 1)]
    for burst in bursts:
        u = C.byref(burst) if burst is not None else None
        for b in (C.byref(bp), None):
            assert plain(None, b, u, d, d, None, None, d, buf.size, d, None, None, None) == EINVAL
            for c in (C.byref(cam), None):
                assert camera(None, b, c, u, d, d, None, None, d, buf.size, d, None, None, None, None, None) == EINVAL
    assert (buf == 0xEE).all()
