"""The device basics every GPU suite needs: the library with its debug entry points declared, the fixture `L`, the option scopes, the
modes, and vectors where a caller keeps them.  Nothing here knows of a solver (tests/_solvers.py, tests/_dist_solvers.py do).

torch and libfastsparse_amd are imported inside the functions: the module itself imports on a machine without a GPU."""
import contextlib
import ctypes as C

import numpy as np
import pytest

FS_OK, FS_ERR_ARG, FS_ERR_NO_TRANSPOSE, FS_ERR_RELEASED = 0, -2, -4, -5     # (test_gpu_dist_pcg.py checks them against the header)
SOLVER_MODES = ("default", "cg_fixed_order=0", "reproducible", "strict_order")
PRODUCT_MODES = ("default", "reproducible", "strict_order")


def lib():
    """capi.lib() with the debug entry points the suites read declared"""
    from libfastsparse_amd import capi
    lib = capi.lib()
    lib.fs_debug_last_cg_state.argtypes = [C.c_void_p]
    lib.fs_debug_last_mscg_state.argtypes = [C.c_void_p, C.c_int]
    lib.fs_debug_last_pcgn_state.argtypes = [C.c_void_p, C.c_int]
    lib.fs_debug_last_mscgn_state.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.fs_debug_dist_products.restype = C.c_long
    lib.fs_debug_dist_products.argtypes = []
    lib.fs_debug_dist_parts.argtypes = [C.c_void_p, C.c_int]
    lib.fs_debug_last_spmm_plan.argtypes = []
    return lib


def gpu_lib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return lib()


@pytest.fixture(scope="module")
def L():
    return gpu_lib()


@contextlib.contextmanager
def options(**kw):
    """set library options, restore the values they had on the way out (an option without a getter would be "restored" to
    FS_ERR_ARG and stay so for the rest of the process: refused)"""
    from libfastsparse_amd import capi
    L = capi.lib()
    old = {k: L.fs_get_option(k.encode()) for k in kw}
    assert all(v != FS_ERR_ARG for v in old.values()), old
    try:
        for k, v in kw.items():
            capi.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            capi.set_option(k, v)


def mode_options(mode):
    """"default" is arrival order, said so: a process started with FS_REPRODUCIBLE=1 runs these tests as well"""
    if mode == "default":
        return options(reproducible=0)
    if mode == "cg_fixed_order=0":
        return options(cg_fixed_order=0)
    return options(**{mode: 1})


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_vector(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def put(a, hbm):
    """a vector where the caller keeps it: host memory, or HBM"""
    a = np.ascontiguousarray(a, np.float64)
    return to_device(a) if hbm else a.copy()


def to_numpy(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else v
