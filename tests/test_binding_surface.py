"""The Python binding's surface, held to a record of it (tests/golden/binding_surface.json): every name the package root
offers and its kind, every ``Structure``'s fields and size, every ``*_DTYPE``'s layout, every integer and tuple
constant, the ``restype`` / ``argtypes`` of every bound function of libaof.so and of the facade library, and the
signature of every function and of every method of the classes callers drive.  CPU only.

``python tests/test_binding_surface.py --record`` writes the record from the package as it stands (in a fresh
process, so that no submodule a test imported shows in it)."""
import ctypes
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_surface.json")
CLASSES = ("FlowEngine", "Bank", "HostOutbox", "_FacadeFlow", "OpticalFlowPX4", "OpticalFlowOpenCV", "OpticalFlowBank")
# the one allowed difference: the package's own modules, which show at its root once something has imported them
SUBMODULES = {"_abi", "_util", "engine", "bank", "facade", "synth", "batch"}


def ctype_repr(t):
    """repr of a restype or of an argtypes list without the defining module's name: ctypes names POINTER(Params)
    ``<class '<module of Params>.LP_Params'>``, and which module of the package defines a record is not surface."""
    return re.sub(r"'[\w.]+\.(\w+)'", r"'\1'", repr(t))


def kind(v):
    if inspect.isclass(v):
        return "class"
    if inspect.ismodule(v):
        return "module"
    if inspect.isfunction(v):
        return "function"
    return "dtype" if isinstance(v, np.dtype) else type(v).__name__


def bound(lib, names):
    return {n: [ctype_repr(getattr(lib, n).restype), ctype_repr(getattr(lib, n).argtypes)] for n in names if hasattr(lib, n)}


def bound_names(lib):
    """The functions a CDLL has handed out so far (it keeps each as an attribute of itself)."""
    return sorted(n for n, v in vars(lib).items() if isinstance(v, ctypes._CFuncPtr))


def members(cls):
    out = {}
    for n in dir(cls):
        if n.startswith("__") and n not in ("__init__", "__del__"):
            continue
        v = inspect.getattr_static(cls, n)
        if isinstance(v, property):
            out[n] = "property " + str(inspect.signature(v.fget))
        elif inspect.isfunction(v):
            out[n] = str(inspect.signature(v))
        else:
            out[n] = kind(v)
    return out


def surface(pkg, with_facade):
    names = {n: getattr(pkg, n) for n in dir(pkg) if not n.startswith("__")}
    s = {
        # (_facade: None until the first facade_lib() of the process, so its kind is not the package's to fix)
        "names": {n: "lazy" if n == "_facade" else kind(v) for n, v in names.items()},
        "structures": {n: {"fields": [[f[0], f[1].__name__] for f in v._fields_], "sizeof": ctypes.sizeof(v)}
                       for n, v in names.items() if inspect.isclass(v) and issubclass(v, ctypes.Structure)},
        "dtypes": {n: {"descr": v.descr, "offsets": {f: v.fields[f][1] for f in v.names}, "itemsize": v.itemsize}
                   for n, v in names.items() if n.endswith("_DTYPE")},
        "constants": {n: v for n, v in names.items() if isinstance(v, (int, tuple))},
        "exports": bound(pkg.lib, pkg.EXPORTS),
        "functions": {n: str(inspect.signature(v)) for n, v in names.items() if inspect.isfunction(v)},
        "methods": {c: members(names[c]) for c in CLASSES},
    }
    if with_facade:
        f = pkg.facade_lib()
        s["facade"] = bound(f, bound_names(f))
    return json.loads(json.dumps(s, sort_keys=True))   # tuples as the file holds them


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_package_surface_is_the_recorded_one(aof, golden):
    now = surface(aof, with_facade=False)
    extra = set(now["names"]) - set(golden["names"])
    assert extra <= SUBMODULES and all(now["names"][n] == "module" for n in extra), sorted(extra)
    for n in extra:
        del now["names"][n]
    assert set(golden["exports"]) == set(aof.EXPORTS)
    for section in ("names", "structures", "dtypes", "constants", "exports", "functions", "methods"):
        assert now[section].keys() == golden[section].keys(), section
        for n in golden[section]:
            assert now[section][n] == golden[section][n], (section, n)


def test_facade_table_is_the_recorded_one(aof, golden):
    if not os.path.exists(aof.FACADE_PATH):
        pytest.skip("facade library not built")
    f = aof.facade_lib()
    assert f is aof.facade_lib(), "loaded once"
    want = golden["facade"]
    assert len(want) >= 40
    now = bound(f, want)
    for n in want:
        assert now.get(n) == want[n], n
    assert set(bound_names(f)) >= set(want)
    typed = {n for n in bound_names(f) if getattr(f, n).argtypes is not None}
    assert typed == set(want), sorted(typed ^ set(want))


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    sys.path.insert(0, ROOT)
    import subprocess
    import __graft_entry__ as ge
    s = surface(ge.load_package(), with_facade=True)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    s = {"_how": "recorded results of this repository's own code: written by `python tests/test_binding_surface.py --record` "
                 f"from the built package at commit {commit}", **s}
    with open(GOLDEN, "w") as f:
        json.dump(s, f, indent=1, sort_keys=True)
        f.write("\n")
    print(GOLDEN, {k: len(v) for k, v in s.items() if isinstance(v, dict)})
