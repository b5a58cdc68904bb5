"""The one rule of how the tests are laid out: a test module is nobody's library.  What several files share lives in a
module that holds no tests (tests/bank_rig.py, tests/bank_cases.py, tests/mavlink_model.py, tests/sequence_ref.py,
tests/npref.py, the *_ref.py models, tests/generic_edges_ref.py: designed inputs and their census)."""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_module_imports_a_test_module():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))
    assert len(files) > 50
    bad = []
    for path in files:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else \
                    [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            bad += [(os.path.relpath(path, ROOT), node.lineno, n) for n in names if n.split(".")[-1].startswith("test_")]
    assert not bad, bad
