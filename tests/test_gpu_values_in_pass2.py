"""The two-pass copy with its values in pass-2 order: pass 1 writes x[col] to the stream, pass 2 loads the entry's value beside it,
multiplies, then adds (fs_kernels_twopass.hip: reduce_panel / spmv_reduce_ordered_kernel / spmm_reduce_kernel, VALUED).

Every case forces the two-pass copy (binning=2, ldsx=0, tiling=0) and compares bits with the exact sums of tests/_exact.py on
exactly summable data (D2 of tests/_large_bands.py: a = +-odd(1..15) x 2^[-4, 4], x and u integers |.| <= 1023), so that the
expected bits come from the oracle CSR product and never from the library.

Shapes
  M  40 000 x 40 000, 8 to 24 entries per row: 3 bands, 4 panels, runs that are no multiples of 16, a partial last pass-2 round
  E  48 000 x 40 000: rows 0 .. 7 999 dense, then nothing for 33 000 rows (one EMPTY PANEL), then 20 rows of 15 entries 300 rows
     apart (a panel of 300 entries, below one 512-entry wave step; row gaps above 255: dummy entries under bin_flags=128); no
     column in 16 384 .. 32 767 (one EMPTY BAND)
  T  the short-run shape of tests/_large_bands.py that makes the builder pick the large-band form (bands of 19 456 columns)
A value that ended up beside another entry's x, a padding or dummy slot that multiplies a real x, a stale value in a tail round:
each changes bits on these data, and with x = +inf everywhere shows up as a NaN."""
import ctypes as C

import numpy as np
import pytest

import _exact as E
import _large_bands as LB
import _plan_model as M

pytestmark = pytest.mark.gpu

options, _d, _poisoned, _eq = LB.options, LB._d, LB._poisoned, LB._eq
FORCE = dict(binning=2, ldsx=0, tiling=0, long_rows=0)
# product-time switches: arrival order, fixed order (the one-wave pass 2), plain loads of products and values (bin_flags bit 8)
RUNS = {"default": {}, "reproducible": dict(reproducible=1), "plain loads": dict(bin_flags=256)}


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"


def _shape_m():
    rng = np.random.default_rng(41)
    n = 40_000
    rows, cols = E._coo(rng.integers(8, 25, n), n, rng)
    return LB._d2("M", n, n, rows, cols, 42)


def _shape_e():
    rng = np.random.default_rng(43)
    nrow, ncol = 48_000, 40_000
    lens = np.zeros(nrow, np.int64)
    lens[:8_000] = 16
    lens[41_000:47_000:300] = 15
    rows = np.repeat(np.arange(nrow), lens)
    cols = rng.integers(0, 16_384 + (ncol - 32_768), rows.size)
    cols[cols >= 16_384] += 16_384                                  # band 1 stays empty
    return LB._d2("E", nrow, ncol, rows, cols, 44)


_DATA, _COPIES = {}, {}


def data(shape, valued):
    if shape not in _DATA:
        d = {"M": _shape_m, "E": _shape_e}[shape]()
        _DATA[shape] = {True: d, False: d.pattern()}
    return _DATA[shape][valued]


def copy_of(shape, ids, valued):
    """the forced two-pass copy of a shape with its A' (ids: bin_flags 64 = two-byte row ids, 128 = one byte), built once"""
    from libfastsparse_amd import capi
    if shape == "T":
        return LB.copy_of("T", valued)
    key = (shape, ids, valued)
    if key not in _COPIES:
        d = data(shape, valued)
        L = LB._lib()
        with options(bin_flags=ids, **FORCE):
            A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), None if d.vals is None else _d(d.vals))
            A.build_transpose(capi.current_stream())
        for t in (0, 1):
            assert A.kernel_name(bool(t)) == "two-pass", (key, t)
            rows8 = L.fs_debug_two_pass_rows8(A.h, t)
            assert (rows8 >= 0) if ids == 128 else (rows8 == -1), (key, t, rows8)
        _COPIES[key] = A
    return _COPIES[key], data(shape, valued)


def _layout(A, t):
    out = (C.c_ulonglong * 8)()
    assert LB._lib().fs_debug_two_pass_layout(A.h, t, out) == 0
    return dict(n=int(out[5]), B=int(out[6]), P=int(out[7]))


def test_shapes_have_the_seams_they_are_named_for(hip):
    """M: 3 bands, several panels, cells that are no multiples of 16 and a panel whose entries are no multiple of a pass-2 round;
    E: an empty band, an empty panel, a panel below 512 entries, dummies under one-byte ids.  Geometry from the planner model."""
    L = LB._lib()
    for shape in ("M", "E"):
        A, d = copy_of(shape, 128, True)
        got = _layout(A, 0)
        vp, cut = M.virtual_rows(d.rp, 256)
        assert not cut
        g = M.plan_two_pass_geometry(d.nrow, d.ncol, d.nnz, 1, 0, LB.bin_env())
        assert g["bcols"] == M.K_BIN_COLS
        panel_row = np.asarray(M.plan_two_pass_panels(vp, d.nrow, d.nnz, g["R"], LB._ncu(), 0.8, 1, 1), np.int64)
        B, P = -(-d.ncol // g["bcols"]), panel_row.size - 1
        assert (got["B"], got["P"]) == (B, P) and B == 3, (shape, got, B, P)
        panel = np.searchsorted(panel_row[:-1], d.rows.astype(np.int64), side="right") - 1
        cells = np.bincount(panel * B + d.cols.astype(np.int64) // g["bcols"], minlength=P * B).reshape(P, B)
        per_panel, per_band = cells.sum(1), cells.sum(0)
        if shape == "M":
            assert P >= 3 and (cells % 16 != 0).any() and (cells > 4096).all()
            assert got["n"] > d.nnz and got["n"] % 16 == 0
        else:
            assert (per_band == 0).any() and (per_panel == 0).any() and ((per_panel > 0) & (per_panel < 512)).any(), (per_panel, per_band)
            assert L.fs_debug_two_pass_rows8(A.h, 0) >= 20, "row gaps above 255: dummy entries"


def _products(A, d, what):
    from libfastsparse_amd import capi
    st = capi.current_stream()
    refs = (d.y(), d.z())
    vs = (_d(d.x), _d(d.u))
    for run, opts in RUNS.items():
        with options(**opts):
            for t in (0, 1):
                assert A.kernel_name(bool(t)) == "two-pass"
                for fill in (float("nan"), -0.0):
                    out = _poisoned((refs[t].size,), fill)
                    A.spmv(out, vs[t], st, transposed=bool(t))
                    _eq(out.cpu().numpy(), refs[t], (what, run, fill, "A' u" if t else "A x"))


@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
@pytest.mark.parametrize("ids", [64, 128], ids=["two-byte ids", "one-byte ids"])
@pytest.mark.parametrize("shape", ["M", "E"])
def test_products_bit_for_bit(hip, shape, ids, valued):
    """A x and A' u: arrival order, fixed order and plain loads, y prefilled with NaN and with -0.0"""
    A, d = copy_of(shape, ids, valued)
    _products(A, d, (shape, ids, valued))


@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
def test_large_band_form_bit_for_bit(hip, valued):
    A, d = copy_of("T", 0, valued)
    _products(A, d, ("T", valued))


@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
@pytest.mark.parametrize("ids", [64, 128], ids=["two-byte ids", "one-byte ids"])
def test_strided_vectors(hip, ids, valued):
    """x and y three doubles apart: k = 3 under spmm_kernel = 3 is one single-vector sweep per column with xs = ys = 3"""
    from libfastsparse_amd import capi
    A, d = copy_of("M", ids, valued)
    L = LB._lib()
    st = capi.current_stream()
    for run in ("default", "reproducible"):
        with options(spmm_kernel=3, **RUNS[run]):
            for t, X, ref in ((0, d.X(3), d.Y(3)), (1, d.U(3), d.Z(3))):
                assert L.fs_matrix_spmm_plan(A.h, 3, t) == LB.BINNED_COLS
                Y = _poisoned(ref.shape, float("nan"))
                A.spmm(Y, _d(X), 3, st, transposed=bool(t))
                _eq(Y.cpu().numpy(), ref, (ids, valued, run, "strided", t))


@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
@pytest.mark.parametrize("shape", ["M", "E"])
def test_k_column_sweeps_equal_the_single_vector_product(hip, shape, valued):
    """k = 2 and k = 4 copies (bands of 8 192 / 4 096 columns, values in THEIR pass-2 order), arrival and fixed order, whole and
    in 3 parts: every column carries the bits of the single-vector product of that column, which are the exact ones"""
    from libfastsparse_amd import capi
    A, d = copy_of(shape, 64, valued)
    st = capi.current_stream()
    for k in (2, 4):
        with options(**FORCE):
            A.prepare(k, st)
        assert A.spmm_plan(k) == "k-column two-pass", (shape, k, A.spmm_plan(k))
        X, ref = d.X(k), d.Y(k)
        Xd = _d(X)
        for run in ("default", "reproducible"):
            with options(**RUNS[run]):
                Y = _poisoned(ref.shape, float("nan"))
                A.spmm(Y, Xd, k, st)
                got = Y.cpu().numpy()
                for j in range(k):
                    y1 = _poisoned((d.nrow,), float("nan"))
                    A.spmv(y1, _d(X[:, j]), st)
                    _eq(got[:, j], y1.cpu().numpy(), (shape, valued, k, run, "column against the single-vector product", j))
                _eq(got, ref, (shape, valued, k, run))
                Y = _poisoned(ref.shape, -0.0)
                for p in range(3):
                    A.spmm_part(Y, Xd, k, p, 3, st)
                _eq(Y.cpu().numpy(), ref, (shape, valued, k, run, "in 3 parts"))


@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
@pytest.mark.parametrize("ids", [64, 128], ids=["two-byte ids", "one-byte ids"])
def test_parts_and_host_vectors(hip, ids, valued):
    """the product in 3 parts (pass 2 by panel ranges) and with host vectors (pass 1 by band ranges, pass 2 by panel ranges)"""
    from libfastsparse_amd import capi
    st = capi.current_stream()
    for shape in ("M", "E"):
        A, d = copy_of(shape, ids, valued)
        for t, v, ref in ((0, d.x, d.y()), (1, d.u, d.z())):
            for run in ("default", "reproducible"):
                with options(**RUNS[run]):
                    y = _poisoned((ref.size,), float("nan"))
                    for p in range(3):
                        A.spmv_part(y, _d(v), p, 3, st, transposed=bool(t))
                    _eq(y.cpu().numpy(), ref, (shape, ids, valued, run, t, "in 3 parts"))
            yh = np.full(ref.size, np.nan)
            A.spmv_host(yh, v, transposed=bool(t))
            _eq(yh, ref, (shape, ids, valued, t, "host vectors"))


def test_pass_1_alone_leaves_the_gathered_x(hip):
    """fs_debug_two_pass_run: pass 1 writes x[col], pass 2 on that stream multiplies and adds -- the whole product; and a stream of
    ones run through pass 2 alone gives the row sums of the values (pass 2 owns the values)"""
    from libfastsparse_amd import capi
    L = LB._lib()
    L.fs_debug_two_pass_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    st = capi.current_stream()
    for ids in (64, 128):
        A, d = copy_of("M", ids, True)
        ones = E.spmv(d.nrow, d.rows, d.cols, d.vals, np.ones(d.ncol))
        for x, ref in ((d.x, d.y()), (np.ones(d.ncol), ones)):
            y = _poisoned((d.nrow,), float("nan"))
            xd = _d(x)
            assert L.fs_debug_two_pass_run(A.h, 0, 1, y.data_ptr(), xd.data_ptr(), st) == 0
            assert np.isnan(y.cpu().numpy()).all(), "pass 1 alone writes no y"
            assert L.fs_debug_two_pass_run(A.h, 0, 2, y.data_ptr(), xd.data_ptr(), st) == 0
            _eq(y.cpu().numpy(), ref, (ids, "pass 1 then pass 2"))


def test_first_fixed_order_product_captured_into_a_graph(hip):
    """a valued one-byte copy whose FIRST fixed-order product is captured: no allocation there, the one-wave pass 2 decodes the
    one-byte ids on the fly (spmv_reduce_ordered_kernel<true, ..., true>) and multiplies"""
    import torch
    from libfastsparse_amd import capi
    d = data("E", True)
    with options(bin_flags=128, **FORCE):
        A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), _d(d.vals))
    assert A.kernel_name() == "two-pass" and LB._lib().fs_debug_two_pass_rows8(A.h, 0) >= 20
    xd, y = _d(d.x), _poisoned((d.nrow,), float("nan"))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with options(reproducible=1):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            A.spmv(y, xd, capi.current_stream())
        g.replay()
        torch.cuda.synchronize()
    _eq(y.cpu().numpy(), d.y(), "captured fixed-order product")
    del g
    A.close()


@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
def test_padding_and_dummies_stay_silent(hip, valued):
    """x = +inf everywhere, positive values: every non-empty row is +inf, every empty row +0.0, nothing is NaN -- a padding or dummy
    slot (value 0) that met a real x would give 0 x inf = NaN.  Every copy, every run, k = 2 and 4, parts, host vectors."""
    from libfastsparse_amd import capi
    st = capi.current_stream()
    for shape, ids in (("M", 64), ("M", 128), ("E", 64), ("E", 128), ("T", 0)):
        _, d = copy_of(shape, ids, valued)
        with options(bin_flags=ids, **FORCE):
            A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), None if valued is False else _d(np.abs(d.vals)))
            A.build_transpose(st)
            if shape != "T":
                for k in (2, 4):
                    A.prepare(k, st)
        want = [np.where(np.bincount(d.rows, minlength=d.nrow) > 0, np.inf, 0.0), np.where(np.bincount(d.cols, minlength=d.ncol) > 0, np.inf, 0.0)]
        for t in (0, 1):
            nin = d.nrow if t else d.ncol
            inf = _poisoned((nin,), float("inf"))
            for run, opts in RUNS.items():
                with options(**opts):
                    assert A.kernel_name(bool(t)) == "two-pass"
                    y = _poisoned((want[t].size,), float("nan"))
                    A.spmv(y, inf, st, transposed=bool(t))
                    _eq(y.cpu().numpy(), want[t], (shape, ids, valued, run, t, "x = +inf"))
                    y = _poisoned((want[t].size,), float("nan"))
                    for p in range(3):
                        A.spmv_part(y, inf, p, 3, st, transposed=bool(t))
                    _eq(y.cpu().numpy(), want[t], (shape, ids, valued, run, t, "x = +inf, in 3 parts"))
            yh = np.full(want[t].size, np.nan)
            A.spmv_host(yh, np.full(nin, np.inf), transposed=bool(t))
            _eq(yh, want[t], (shape, ids, valued, t, "x = +inf, host vectors"))
        if shape != "T":
            for k in (2, 4):
                assert A.spmm_plan(k) == "k-column two-pass"
                for run in ("default", "reproducible"):
                    with options(**RUNS[run]):
                        Y = _poisoned((d.nrow, k), float("nan"))
                        A.spmm(Y, _poisoned((d.ncol, k), float("inf")), k, st)
                        _eq(Y.cpu().numpy(), np.repeat(want[0][:, None], k, 1), (shape, ids, valued, run, k, "X = +inf"))
        A.close()
