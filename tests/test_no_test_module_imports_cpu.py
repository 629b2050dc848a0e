"""No module under tests/ or tools/ imports a test module: what several suites share lives in a helper module
(tests/guarded_launch.py, tests/host_helpers.py, tests/plan_jvp_model_checks.py, the *_cases.py and *_np.py files), so running
one file imports no other file's tests and module-level state."""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _imported_modules(path):
    """(line, module) of every import statement of a file, those inside functions included"""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for alias in node.names:
                yield node.lineno, alias.name
        elif isinstance(node, ast.ImportFrom) and node.module:
            yield node.lineno, node.module


def test_no_module_imports_a_test_module():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))
    assert any(path.endswith("guarded_launch.py") for path in files), "the glob found no module under tests/"
    bad = [(os.path.relpath(path, ROOT), line, module) for path in files for line, module in _imported_modules(path)
           if any(part.startswith("test_") for part in module.split("."))]
    assert not bad, bad
