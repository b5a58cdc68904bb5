"""The rig of the sanitized native programs (tests/native/*.cpp, each with its own main): one recipe to build one and to run
it, and the record by which a plan model (tests/*_plan_ref.py) hands a family of cases to tests/test_host_asan.py.  CPU only;
nothing here is loaded into Python."""
import collections
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "aero-optical-flow_amd/csrc"
TIMEOUT_S = 300


def build(out_dir, name, sources, *, fp_contract_off=False, float_cast=False, hip_host=False, extra_includes=()):
    """Compiles `sources` (paths below the repository root) into out_dir/name under ASan and UBSan, with include/ and csrc/ as
    include directories, and returns the program's path.  The compiler is $CXX (default c++); hip_host: $HIPCC (default
    /opt/rocm/bin/hipcc) on the sources as host C++, the way the library's Makefile compiles a host-only translation unit."""
    exe = os.path.join(str(out_dir), name)
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc") if hip_host else os.environ.get("CXX", "c++"), "-O1", "-g", "-std=c++17"]
    if hip_host:
        cmd += ["-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
    if fp_contract_off:
        cmd.append("-ffp-contract=off")
    cmd.append("-fsanitize=address,undefined")
    if float_cast:
        cmd.append("-fsanitize=float-cast-overflow")
    cmd += ["-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, CSRC)]
    cmd += ["-I" + os.path.join(ROOT, d) for d in extra_includes] + [os.path.join(ROOT, s) for s in sources] + ["-o", exe]
    subprocess.run(cmd, check=True, timeout=TIMEOUT_S)
    return exe


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=TIMEOUT_S)


# One family of a plan model for `host_selftest <check> <listing>`: the listing holds line(c) for every c of cases (dicts with an
# id); the program prints one line that starts with `tag` per case, whose integers are want(c) under `names`, and `summary` with
# the number of cases in it.  Two families may share a check (one listing, one run, two tags).
Family = collections.namedtuple("Family", "name check tag summary cases line want names")


def family(check, tag, cases, line, want, names, name=None, summary=None):
    return Family(name or check, check, tag, summary or tag + "{} cases", cases, line, want, names)


def joined(values):
    return " ".join(str(v) for v in values)
