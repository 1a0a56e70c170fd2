"""Every kernel path, bit for bit, on exactly summable data (tests/_exact.py).

On these data every product and every partial sum is exact, so every order of additions -- arrival order, trees, atomics, parts,
ranks -- must give the exact sum, with +0.0 for a zero sum, in the default mode, under "reproducible" and under "strict_order"
alike.  The 1e-12 row-scaled bar of the parity tests cannot see a dropped 2^-46 term, a flushed subnormal or a -0.0; these tests
can.  Each test also asserts that the path it is named for really ran (kernel_name, spmm_plan, the debug hooks)."""
import ctypes as C

import numpy as np
import pytest

import _cases
import _exact as E
from _exact import PATHS
from _gpu import PRODUCT_MODES as MODES, mode_options as _mode, options, to_device as _d

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import _hipbackend as H
    return H


def _poisoned(shape, fill):
    import torch
    return torch.full(shape, fill, dtype=torch.float64, device="cuda")


def _eq(got, want, what):
    assert E.bits_equal(got, want), f"{what}: {E.first_mismatch(got, want)}"


SETS = {d.name: d for d in (E.wide_range(), E.long_rows(profile="heavy", nrow=4000, seed=6), E.subnormal(), E.subnormal_pattern(),
                            E.zeros(), E.zeros(valued=False))}
EXPECT = {n: (d.y(), d.z()) for n, d in SETS.items()}


def _build(d, path):
    from libfastsparse_amd import capi
    opts, _ = PATHS[path]
    with options(**opts):
        A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), None if d.vals is None else _d(d.vals))
        A.build_transpose(capi.current_stream())
    return A


def _assert_path(A, path, mode, transposed=False):
    """the forced copy ran: by name, and by the debug hooks where a name does not tell the forms apart"""
    from libfastsparse_amd import capi
    L = capi.lib()
    want = PATHS[path][1]
    if mode == "strict_order":
        want = "stream"
    elif mode == "reproducible" and want == "lds-staged":
        L.fs_debug_ldsx_orderable.argtypes = [C.c_void_p, C.c_int]
        if L.fs_debug_ldsx_orderable(A.h, int(transposed)) != 1:
            want = "stream"                          # the documented fallback of a copy that cannot be ordered
    assert A.kernel_name(transposed) == want, (path, mode, transposed, A.kernel_name(transposed))
    if want != "two-pass":
        return
    L.fs_debug_two_pass_rows8.restype = C.c_longlong
    L.fs_debug_two_pass_rows8.argtypes = [C.c_void_p, C.c_int]
    rows8 = L.fs_debug_two_pass_rows8(A.h, int(transposed))
    if path != "long rows":                          # (the long-row copy keeps the form the builder picks for its rows)
        assert (rows8 >= 0) if path == "two-pass one-byte" else (rows8 == -1), (path, rows8)
    if path == "long rows" and not transposed:
        info = (C.c_int64 * 2)()
        L.fs_debug_long_rows.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
        assert L.fs_debug_long_rows(A.h, 0, info) == 0 and info[0] > 0, info[0]


@pytest.mark.parametrize("path", [p for p in PATHS if p != "long rows"])
@pytest.mark.parametrize("name", list(SETS))
def test_single_vector_paths_are_exact(hip, name, path):
    """A x and A' u on every forced copy, three modes, y prefilled with NaN and -0.0; products in 3 parts; host vectors.
    The LDS-staged copy runs with x aligned (LDS DMA) and with x 8 bytes off (the register form)."""
    from libfastsparse_amd import capi
    d = SETS[name]
    y_ref, z_ref = EXPECT[name]
    A = _build(d, path)
    st = capi.current_stream()
    xd, ud = _d(d.x), _d(d.u)
    xoff = _poisoned((d.ncol + 1,), 0.0)
    xoff[1:] = xd
    for mode in MODES:
        with _mode(mode):
            _assert_path(A, path, mode)
            _assert_path(A, path, mode, transposed=True)
            for fill in (float("nan"), -0.0):
                y, z = _poisoned((d.nrow,), fill), _poisoned((d.ncol,), fill)
                A.spmv(y, xd, st)
                A.spmv(z, ud, st, transposed=True)
                _eq(y.cpu().numpy(), y_ref, (name, path, mode, fill, "A x"))
                _eq(z.cpu().numpy(), z_ref, (name, path, mode, fill, "A' u"))
            if path == "lds-staged":
                y = _poisoned((d.nrow,), float("nan"))
                A.spmv(y, xoff[1:], st)
                _eq(y.cpu().numpy(), y_ref, (name, path, mode, "A x, x 8 bytes off"))
            y = _poisoned((d.nrow,), float("nan"))
            for part in range(3):
                A.spmv_part(y, xd, part, 3, st)
            _eq(y.cpu().numpy(), y_ref, (name, path, mode, "A x in 3 parts"))
            yh, zh = np.full(d.nrow, np.nan), np.full(d.ncol, np.nan)
            A.spmv_host(yh, d.x)
            A.spmv_host(zh, d.u, transposed=True)
            _eq(yh, y_ref, (name, path, mode, "host vectors"))
            _eq(zh, z_ref, (name, path, mode, "host vectors, A' u"))
            if path == "lds-staged" and mode == "reproducible":
                # exact data cannot show the ORDER of additions: no chunk of an orderable copy may have given up waiting its turn
                L = capi.lib()
                L.fs_debug_ldsx_orderable.argtypes = [C.c_void_p, C.c_int]
                L.fs_debug_ldsx_ticket_giveups.argtypes = [C.c_void_p, C.c_int]
                for t in (0, 1):
                    if L.fs_debug_ldsx_orderable(A.h, t) == 1:
                        assert L.fs_debug_ldsx_ticket_giveups(A.h, t) == 0, (name, t)


@pytest.mark.parametrize("name", ["long_rows_heavy", "subnormal"])
def test_long_rows_are_exact(hip, name):
    """the long-row path (rows of >= 32 entries out of the two-pass copy, on a copy of >= 4 M entries): A x in three modes, in
    3 parts, host vectors; integers on rows of up to 50 000 entries, and subnormal products"""
    from libfastsparse_amd import capi
    if name == "subnormal":
        d = E.subnormal(nrow=130_000, ncol=100_000, seed=9)
    else:
        d = E.long_rows(profile="heavy", nrow=150_000, ncol=200_000, seed=8)
    ref = d.y()
    A = _build(d, "long rows")
    st = capi.current_stream()
    for mode in MODES:
        with _mode(mode):
            _assert_path(A, "long rows", mode)
            for fill in (float("nan"), -0.0):
                y = _poisoned((d.nrow,), fill)
                A.spmv(y, _d(d.x), st)
                _eq(y.cpu().numpy(), ref, (name, mode, fill))
            y = _poisoned((d.nrow,), float("nan"))
            for part in range(3):
                A.spmv_part(y, _d(d.x), part, 3, st)
            _eq(y.cpu().numpy(), ref, (name, mode, "in 3 parts"))
            yh = np.full(d.nrow, np.nan)
            A.spmv_host(yh, d.x)
            _eq(yh, ref, (name, mode, "host vectors"))


def test_lds_staged_copy_that_cannot_be_ordered_is_exact(hip):
    """dense rows (300 entries of a row inside one work item): the kept LDS-staged copy is not orderable; under the solvers' wish
    (cg_fixed_order) it keeps running in arrival order, under "reproducible" the product leaves it for the chunk-streaming kernel;
    both exact on subnormal x"""
    from libfastsparse_amd import capi
    L = capi.lib()
    L.fs_debug_ldsx_orderable.argtypes = [C.c_void_p, C.c_int]
    L.fs_debug_fixed_order_honoured.argtypes = [C.c_void_p, C.c_int]
    nrow, ncol, per = 6000, 2048, 300
    rng = np.random.default_rng(300)
    rows = np.repeat(np.arange(nrow), per)
    cols = rng.integers(0, ncol, rows.size)
    x = np.where(rng.uniform(size=ncol) < 0.5, -1.0, 1.0) * np.ldexp(1.0, rng.integers(-1060, -1030, ncol))
    d = E.Data("dense_rows", nrow, ncol, rows, cols, None, x, np.ones(nrow), lambda j: x)
    ref = d.y()
    with options(ldsx=2):
        A = capi.Matrix.from_csr(nrow, ncol, _d(d.rp), _d(d.cols), None)
    with _mode("default"):
        assert A.kernel_name() == "lds-staged" and L.fs_debug_ldsx_orderable(A.h, 0) == 0
    st = capi.current_stream()
    for opts, want in ((dict(cg_fixed_order=1, reproducible=0), "lds-staged"), (dict(reproducible=1), "stream"), (dict(strict_order=1), "stream")):
        with options(**opts):
            assert A.kernel_name() == want, (opts, A.kernel_name())
            y = _poisoned((nrow,), float("nan"))
            A.spmv(y, _d(x), st)
            _eq(y.cpu().numpy(), ref, opts)
    with _mode("default"):
        assert L.fs_debug_fixed_order_honoured(A.h, 0) == 0


def _holes(valued, seed=11):
    """one 16 384-row panel with long empty stretches: row steps far above 255 are walked by dummy entries in the one-byte form"""
    rng = np.random.default_rng(seed)
    nrow, ncol = 40_000, 5_000
    lens = np.zeros(nrow, np.int64)
    lens[:10_000], lens[16_000], lens[30_000:30_010], lens[39_999] = 3, 2, 5, 1
    rows = np.repeat(np.arange(nrow), lens)
    cols = rng.integers(0, ncol, rows.size)
    vals = np.where(rng.uniform(size=rows.size) < 0.5, -1.0, 1.0) * np.ldexp(1.0, rng.integers(-1040, -1030, rows.size) + 530) if valued else None
    x = np.where(rng.uniform(size=ncol) < 0.5, -1.0, 1.0) * np.ldexp(1.0, rng.integers(-540, -530, ncol))
    if not valued:
        x = x * 2.0 ** -500
    return E.Data("holes", nrow, ncol, rows, cols, vals, x, np.ones(nrow), lambda j: x)


@pytest.mark.parametrize("valued", [True, False])
def test_one_byte_row_ids_with_holes_exact_and_non_finite(hip, valued):
    """the one-byte-id copy with dummy entries: subnormal products exact in three modes; then NaN / +inf in x reach exactly the
    rows that reference those columns (a dummy entry of value 0 must not carry them anywhere)"""
    from libfastsparse_amd import capi
    L = capi.lib()
    L.fs_debug_two_pass_rows8.restype = C.c_longlong
    L.fs_debug_two_pass_rows8.argtypes = [C.c_void_p, C.c_int]
    d = _holes(valued)
    with options(binning=2, ldsx=0, tiling=0, bin_flags=128):
        A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), None if d.vals is None else _d(d.vals))
    assert A.kernel_name() == "two-pass" and L.fs_debug_two_pass_rows8(A.h, 0) >= 20
    st = capi.current_stream()
    ref = d.y()
    assert (ref != 0).sum() > 1000 and np.all(np.abs(ref) < 2.0 ** -1000)
    for mode in MODES:
        with _mode(mode):
            y = _poisoned((d.nrow,), float("nan"))
            A.spmv(y, _d(d.x), st)
            _eq(y.cpu().numpy(), ref, (mode, "holes"))
    x = d.x.copy()
    x[[17, 2500]], x[4000] = np.nan, np.inf
    for mode in MODES:
        with _mode(mode):
            y = _poisoned((d.nrow,), -0.0)
            A.spmv(y, _d(x), st)
            got = y.cpu().numpy()
            hit_nan = np.zeros(d.nrow, bool)
            np.logical_or.at(hit_nan, d.rows, np.isin(d.cols, [17, 2500]))
            hit_inf = np.zeros(d.nrow, bool)
            np.logical_or.at(hit_inf, d.rows, d.cols == 4000)
            assert hit_nan.sum() > 0 and hit_inf.sum() > 0
            bad = hit_nan | hit_inf
            assert np.array_equal(~np.isfinite(got), bad), (mode, np.flatnonzero(~np.isfinite(got) != bad)[:5])
            assert np.all(np.isnan(got[hit_nan])), mode
            _eq(got[~bad], ref[~bad], (mode, "finite rows beside non-finite x"))


@pytest.fixture(scope="module")
def dense_cells():
    """the dense-cell one-byte shape (hundreds of entries per (band, panel) cell, as config 2), long-row integers: built once"""
    rng = np.random.default_rng(12)
    nrow = ncol = 300_000
    rows = np.repeat(np.arange(nrow), 16)
    cols = rng.integers(0, ncol, rows.size)
    vals = np.where(rng.uniform(size=rows.size) < 0.5, -1.0, 1.0) * np.ldexp((2 * rng.integers(0, 8, rows.size) + 1).astype(float),
                                                                             rng.integers(-4, 5, rows.size))
    x = rng.integers(-1023, 1024, ncol).astype(np.float64)
    d = E.Data("dense_cells", nrow, ncol, rows, cols, vals, x, rng.integers(-1023, 1024, nrow).astype(np.float64), lambda j: x)
    return d, d.y(), d.z()


def test_one_byte_row_ids_dense_cells(hip, dense_cells):
    from libfastsparse_amd import capi
    L = capi.lib()
    L.fs_debug_two_pass_rows8.restype = C.c_longlong
    L.fs_debug_two_pass_rows8.argtypes = [C.c_void_p, C.c_int]
    d, y_ref, z_ref = dense_cells
    with options(binning=2, bin_flags=128):
        A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), _d(d.vals))
        A.build_transpose(capi.current_stream())
    assert A.kernel_name() == "two-pass" and 0 <= L.fs_debug_two_pass_rows8(A.h, 0) <= 0.01 * d.nnz
    st = capi.current_stream()
    for mode in MODES:
        with _mode(mode):
            y, z = _poisoned((d.nrow,), float("nan")), _poisoned((d.ncol,), float("nan"))
            A.spmv(y, _d(d.x), st)
            A.spmv(z, _d(d.u), st, transposed=True)
            _eq(y.cpu().numpy(), y_ref, (mode, "A x"))
            _eq(z.cpu().numpy(), z_ref, (mode, "A' u"))


# ---- k columns ---------------------------------------------------------------------------------------------------
SPMM_SETS = ("wide_range", "subnormal", "zeros")


@pytest.mark.parametrize("name", SPMM_SETS)
def test_k_columns_every_kernel_is_exact(hip, name):
    """the k-column two-pass sweep (k = 2, 3, 4, prepared and not), the row kernel (k = 5, 8, 32, 40; 16-byte loads with
    spmm_wide), the MFMA experiment, products in parts: all against the exact reference, three modes"""
    from libfastsparse_amd import capi
    d = SETS[name]
    st = capi.current_stream()
    with options(binning=2):
        A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), None if d.vals is None else _d(d.vals))
    assert A.kernel_name() == "two-pass"

    def run(k, what, want_plan=None, parts=False):
        X = d.X(k)
        ref = d.Y(k)
        for mode in MODES:
            with _mode(mode):
                if want_plan and mode == "default":
                    assert A.spmm_plan(k) == want_plan, (what, k, A.spmm_plan(k))
                Y = _poisoned((d.nrow, k), float("nan"))
                A.spmm(Y, _d(X), k, st)
                _eq(Y.cpu().numpy(), ref, (name, what, k, mode, A.spmm_plan(k)))
                if parts:
                    Y = _poisoned((d.nrow, k), -0.0)
                    for p in range(3):
                        A.spmm_part(Y, _d(X), k, p, 3, st)
                    _eq(Y.cpu().numpy(), ref, (name, what, k, mode, "in 3 parts"))

    for k in (2, 3, 4):                              # before any prepare: what the handle holds
        run(k, "unprepared", "two-pass per column" if k <= 3 else "row")
    for k in (2, 3, 4):
        with options(binning=2):
            A.prepare(k, st)
        run(k, "k-column sweep", "k-column two-pass", parts=True)
    for k in (5, 8, 32, 40):
        with options(spmm_kernel=1):
            run(k, "row kernel", "row")
            with options(spmm_wide=1):
                run(k, "row kernel, 16-byte loads", "row")
    with options(binning=0, ldsx=0, tiling=0):      # the MFMA experiment runs on the plain CSR of a handle without a kept copy
        A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), None if d.vals is None else _d(d.vals))
    assert A.kernel_name() == "stream"
    for k in (2, 4, 40):
        with options(spmm_kernel=4):
            run(k, "mfma", "mfma")


@pytest.mark.parametrize("name", ["subnormal_pattern", "ata_ints"])
def test_fused_ata_is_exact(hip, name):
    """y = A'A x: the two products (ata_kernel 0), the fused kernel (ata_kernel 2) on the plain CSR and on the LDS-staged copy.
    No debug hook reports which A'A form ran: the option forces it, and the copy it runs on is asserted by name."""
    from libfastsparse_amd import capi
    if name == "ata_ints":
        d = E.long_rows(seed=21, nrow=3000, ncol=2000, maxlen=200)
    else:
        d = SETS[name]
    ref = E.ata(d.nrow, d.ncol, d.rows, d.cols, d.vals, d.x)
    st = capi.current_stream()
    for create, want in ((dict(binning=0, ldsx=0, tiling=0), "stream"), (dict(ldsx=2, binning=0, tiling=0, tile_rows=512), "lds-staged")):
        with options(**create):
            A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), None if d.vals is None else _d(d.vals))
        with _mode("default"):
            assert A.kernel_name() == want
        tmp = _poisoned((d.nrow,), float("nan"))
        for ata_kernel in (0, 2):
            for mode in MODES:
                with options(ata_kernel=ata_kernel), _mode(mode):
                    y = _poisoned((d.ncol,), float("nan"))
                    A.ata(y, _d(d.x), tmp, st)
                    _eq(y.cpu().numpy(), ref, (name, want, ata_kernel, mode))


@pytest.mark.parametrize("nnz_per_row", [6, 20])
def test_cbcsr_cell_streaming_and_general_path_are_exact(hip, nnz_per_row):
    """the column-blocked binary form at >= 1 M entries (cell streaming) and >= 4 M (general path), subnormal x.  No debug hook
    reports which path the automatic choice (spmv_kernel 0) took, so each path is also forced, as the parity tests do: the
    one-thread-per-row kernels (spmv_kernel 5, 4) and, on the larger matrix, the cell-streaming path (9)."""
    from libfastsparse_amd import capi
    from oracle import pyoracle as O
    nrow, ncol, cbs = 210_000, 300_000, 65536
    rng = np.random.default_rng(nnz_per_row)
    rows = np.repeat(np.arange(nrow, dtype=np.int32), nnz_per_row)
    cols = rng.integers(0, ncol, rows.size).astype(np.int32)
    x = np.where(rng.uniform(size=ncol) < 0.5, -1.0, 1.0) * np.ldexp(3.0, rng.integers(-1064, -1028, ncol))
    ref = E.cbcsr(nrow, rows, cols, x)
    nb, crp, ccc = O.coo_to_cbcsr(cbs, nrow, ncol, rows, cols)
    m = capi.ColBlockMatrix(nrow, ncol, nb, cbs, _d(crp), _d(ccc))
    for mode in MODES:
        for kernel in ((0, 9, 5) if nnz_per_row == 20 else (0, 5, 4)):
            with _mode(mode), options(spmv_kernel=kernel):
                y = _poisoned((nrow,), float("nan"))
                m.spmv(y, _d(x), capi.current_stream())
                _eq(y.cpu().numpy(), ref, (mode, kernel))


# ---- every reference-named entry point ------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["device", "dropin"])
@pytest.mark.parametrize("name", ["wide_range", "long_rows_single", "zeros"])
def test_every_entry_point_on_host_structs_is_exact(hip, backend, name):
    data = {"wide_range": SETS["wide_range"], "long_rows_single": E.long_rows(nrow=1500), "zeros": SETS["zeros"]}[name]
    case = data.case()
    want = _cases.run_case(E.ExactBackend(), case)
    be = hip.HipDeviceBackend() if backend == "device" else hip.HipDropinBackend()
    for mode in MODES:
        with _mode(mode):
            got = _cases.run_case(be, case)
        assert got.keys() == want.keys()
        bad = [f"{k}: {E.first_mismatch(got[k], want[k])}" for k in sorted(got) if not E.bits_equal(got[k], want[k])]
        assert not bad, (name, backend, mode, bad)


# ---- several ranks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wide_range", "subnormal", "zeros"])
def test_native_context_on_three_virtual_ranks_is_exact(hip, name):
    from libfastsparse_amd import capi
    L = capi.lib()
    d = SETS[name]
    y_ref, z_ref = EXPECT[name]
    vals = None if d.vals is None else d.vals
    devs = (C.c_int * 3)(0, 0, 0)
    D = L.fs_dist_create(3, devs)
    assert D, L.fs_last_error()
    try:
        with options(binning=2, bin_rows=256):
            M = L.fs_dist_csr_create(D, d.nrow, d.ncol, d.nnz, d.rp.ctypes.data, d.cols.ctypes.data, None if vals is None else vals.ctypes.data)
            assert M, L.fs_last_error()
            assert L.fs_dist_matrix_build_transpose(M, d.rp.ctypes.data, d.cols.ctypes.data, None if vals is None else vals.ctypes.data) == 0
        try:
            for mode in MODES:
                with _mode(mode):
                    y, z = np.full(d.nrow, np.nan), np.full(d.ncol, np.nan)
                    assert L.fs_dist_spmv(M, y.ctypes.data, d.x.ctypes.data) == 0, L.fs_last_error()
                    assert L.fs_dist_spmv_t(M, z.ctypes.data, d.u.ctypes.data) == 0, L.fs_last_error()
                    _eq(y, y_ref, (name, mode, "A x, 3 ranks"))
                    _eq(z, z_ref, (name, mode, "A' u, 3 ranks"))
        finally:
            L.fs_dist_matrix_destroy(M)
    finally:
        L.fs_dist_destroy(D)


def test_dropin_across_three_ranks_in_a_child_process_is_exact(hip):
    """FASTSPARSE_NGPU=3 FASTSPARSE_DEVICES=0,0,0: every reference-named entry point of the drop-in on the row-sharded path, with
    the exact data sets, bit for bit; tests/_dropin_ngpu.py (mode `exact`) is the child, a fresh process because the library reads
    the variables once"""
    import os
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dropin_ngpu.py")
    env = dict(os.environ, FASTSPARSE_NGPU="3", FASTSPARSE_DEVICES="0,0,0")
    p = subprocess.run([sys.executable, child, "exact"], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), p.stdout[-3000:] + p.stderr[-3000:]
