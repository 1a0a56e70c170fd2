"""The large-band form of the two-pass copy (bands of 19 456 columns, panels of up to 19 456 rows: the form every config-5 shard
runs on), bit for bit at its seams: local column and row ids above 16 383, a last band that is no multiple of 1 024 columns, cells
of whole rounds plus a padded rest, in every mode, in parts, with host vectors, with strided vectors, with non-finite x and on
data that round.  Its kernel instantiations (fs_kernels_twopass.hip, `N.bcols == kBinColsBig`) are reached nowhere else but on
trivial matrices and at full size.

Shapes, expected values (tests/_exact.py) and the cases live in tests/_large_bands.py; tests/test_large_bands_shapes.py holds the
shapes to what they claim on the CPU.  T runs in this process: the builder picks the form by itself.  D needs FS_BIN_BIG=1, which
the library reads once per process, so all of D's cases run in ONE fresh child (tests/_large_bands.py as a program), started once;
every case is then asserted by itself from the child's `OK <case>` / `FAIL <case>: <message>` lines.  Every case asserts that the
form ran (kernel name, band and panel counts against the planner's, two-byte row ids) before it trusts a result."""
import os
import subprocess
import sys
import time

import pytest

import _large_bands as LB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"


@pytest.mark.parametrize("case", list(LB.T_CASES))
def test_thin_shape_in_process(gpu, case):
    """T, the form picked by the builder itself: see the case's docstring in tests/_large_bands.py"""
    t0 = time.time()
    LB.run(case)
    print(f"{case}: {time.time() - t0:.2f} s")


@pytest.fixture(scope="module")
def child(gpu):
    """every case of D and the long-row case in one fresh process with FS_BIN_BIG=1: {case: (ok, message)}, and the output"""
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(LB.__file__)), "_large_bands.py")] + list(LB.D_CASES),
                       env=dict(os.environ, FS_BIN_BIG="1"), capture_output=True, text=True, timeout=600)
    print(f"the FS_BIN_BIG=1 child took {time.time() - t0:.1f} s\n{p.stdout[-4000:]}")
    seen = {}
    for line in p.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word == "OK":
            seen[rest.strip()] = (True, "")
        elif word == "FAIL":
            name, _, msg = rest.partition(": ")
            seen[name.strip()] = (False, msg)
    return seen, p


@pytest.mark.parametrize("case", list(LB.D_CASES))
def test_dense_shape_in_a_fresh_process(child, case):
    """D (and the long-row set) with the form forced: the child's verdict on this case.  A case the child never reached -- it stops
    at the first failure -- fails too, with the child's last output."""
    seen, p = child
    assert case in seen, (case, "not reached", p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    ok, msg = seen[case]
    assert ok, (case, msg, p.stderr[-3000:])


def test_the_child_ended_clean(child):
    seen, p = child
    assert p.returncode == 0 and set(seen) == set(LB.D_CASES) and all(ok for ok, _ in seen.values()), (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
