"""What hipcc makes of a kernel source file, for the tests that hold kernels to a census, a register budget or a pinned
hash (tests/test_bank_kernel_budgets.py, tests/test_isa_hashes.py): tools/isa_hashes.py, loaded once, and its kernels_of()
per file of aero-optical-flow_amd/csrc, compiled once per process.  hipcc cross-compiles gfx950 without a GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_hashes", os.path.join(ROOT, "tools", "isa_hashes.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

_kernels = {}


def kernels(name):
    """{kernel: (name, hash, vgprs, vgpr spills, sgpr spills, scratch bytes)} of one source file."""
    if name not in _kernels:
        _kernels[name] = {k[0]: k for k in tool.kernels_of(os.path.join(tool.CSRC, name))}
    return _kernels[name]
