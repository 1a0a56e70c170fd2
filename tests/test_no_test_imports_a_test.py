"""The suites share their helpers through the harness (tests/_gpu.py, _solvers.py, _dist_solvers.py), never through each other: no
module under tests/ imports a test_* module, at any depth.  One pair is allowed: the child process _dropin_ngpu.py runs the CASES and
_check of test_gpu_parity.py.  The harness modules import neither torch nor libfastsparse_amd at module level, so the CPU-only
collection imports them on a machine without a GPU.  Reads source only."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ALLOWED = {("_dropin_ngpu.py", "test_gpu_parity")}
HARNESS = ("_gpu.py", "_solvers.py", "_dist_solvers.py")
DEVICE_ONLY = ("torch", "libfastsparse_amd")


def _imports(nodes):
    """(module name, line) of every import statement among the nodes"""
    out = []
    for n in nodes:
        if isinstance(n, ast.Import):
            out += [(a.name, n.lineno) for a in n.names]
        elif isinstance(n, ast.ImportFrom):
            out.append((n.module or "", n.lineno))
    return out


def _tree(name):
    with open(os.path.join(HERE, name)) as f:
        return ast.parse(f.read(), name)


def test_no_module_imports_a_test_module():
    files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(HERE, "*.py")))
    assert len(files) > 50 and set(HARNESS) <= set(files), files
    found = {(f, m.split(".")[0]) for f in files for m, _ in _imports(ast.walk(_tree(f))) if m.split(".")[0].startswith("test_")}
    assert found == ALLOWED, sorted(found ^ ALLOWED)


def test_the_harness_imports_without_a_gpu():
    for f in HARNESS:
        bad = [(m, line) for m, line in _imports(_tree(f).body) if m.split(".")[0] in DEVICE_ONLY]
        assert not bad, (f, bad)
