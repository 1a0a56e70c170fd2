"""Every multi-column product plan (spmm_plan, libfastsparse_amd/csrc/fs_kernels.hip) on A and on A', bit for bit.

One table, TABLE, names for each case the copy forced when the matrix and its A' are built, the side, whether fs_matrix_prepare ran,
the product-time options, the ks, and the plan spmm_plan must choose in each mode.  Every case asserts that plan before it trusts a
result, and then checks:
  exact data (tests/_exact.py, valued and pattern-only): fs_spmm / fs_spmm_t and fs_spmm_part in 1, 3 and 7 parts give the exact
      A X(k) / A' U(k) in all three modes, outputs prefilled with NaN and with -0.0;
  non-exact data (sin X and U; the pattern-only matrix and the pattern with sin values): under strict_order the oracle's storage-order bits (csr_mul_n on A, coo_tmul per column on A');
      under reproducible five runs and the parts give the same bits; by default the 1e-12 row-scaled bar per column.  The row
      kernel adds in storage order in every mode, so wherever it runs its bits are the oracle's.
Then: layout branches of the row kernel, degenerate matrices, the drop-in's k-column entry points and a captured graph."""
import collections
import ctypes as C

import numpy as np
import pytest

import _cases
import _exact as E
from _gpu import PRODUCT_MODES as MODES, mode_options as _mode, options, to_device as _d

ROW, BINNED_K, BINNED_COLS, MFMA, LDSX_COLUMNS, LDSX_STRIDED, TILED_STRIDED = range(1, 8)   # fs_matrix_spmm_plan codes

# forced copy -> (options around fs_csr_create AND fs_matrix_build_transpose, fs_matrix_spmv_kernel name)
COPIES = {
    "none": (dict(binning=0, ldsx=0, tiling=0), "stream"),
    "two-pass": (dict(binning=2, ldsx=0, tiling=0), "two-pass"),
    "lds-staged": (dict(ldsx=2, binning=0, tiling=0), "lds-staged"),
    "tiled": (dict(tiling=2, binning=0, ldsx=0), "tiled"),
    "tiled cut rows": (dict(tiling=2, binning=0, ldsx=0, tile_rows=64, tile_cols=128, tile_split=5), "tiled"),
}

Case = collections.namedtuple("Case", "copy prepared opts ks plans sets")
# plans: (default, reproducible, strict_order); a pair (p, q) under reproducible: p on an LDS-staged copy that can be ordered
# (fs_debug_ldsx_orderable), q on one that cannot.  Every mode's plan follows spmm_plan's rules:
#   strict_order skips every free-order plan and the MFMA experiment: the row kernel, always;
#   reproducible keeps the two-pass plans (their pass 2 runs in stream order), the L2-tiled one and MFMA (fixed per-row
#   orders), the LDS-staged ones only on a copy that can be ordered.
_R = (ROW, ROW, ROW)
_ODD = ("wide_range", "wide_range_odd")
ROWS = [
    Case("none", False, {}, (2, 3, 5, 17, 33, 130), _R, ("wide_range",)),
    Case("none", False, dict(spmm_kernel=4), (2, 5, 33), (MFMA, MFMA, ROW), ("wide_range",)),
    Case("two-pass", False, {}, (2, 3), (BINNED_COLS, BINNED_COLS, ROW), ("wide_range",)),
    Case("two-pass", False, {}, (4, 5, 16), _R, ("wide_range",)),
    Case("two-pass", False, dict(spmm_kernel=4), (4, 8), (MFMA, MFMA, ROW), ("wide_range",)),
    Case("two-pass", True, {}, (2, 3, 4), (BINNED_K, BINNED_K, ROW), _ODD),
    Case("two-pass", True, dict(spmm_kernel=3), (4, 5, 8), (BINNED_COLS, BINNED_COLS, ROW), ("wide_range",)),
    Case("two-pass", True, dict(spmm_kernel=1, spmm_wide=1), (2, 4, 8, 32, 64, 3, 65), _R, ("wide_range",)),
    Case("lds-staged", False, {}, (2,), (LDSX_STRIDED, (LDSX_STRIDED, ROW), ROW), _ODD),
    Case("lds-staged", False, {}, (3, 5), _R, ("wide_range",)),
    Case("lds-staged", True, {}, (2,), (LDSX_COLUMNS, (LDSX_COLUMNS, ROW), ROW), _ODD),
    Case("lds-staged", True, dict(spmm_kernel=3), (3, 4, 5, 8, 16), (LDSX_COLUMNS, (LDSX_COLUMNS, ROW), ROW), _ODD),
    Case("lds-staged", True, {}, (17, 33), _R, ("wide_range",)),
    Case("tiled", False, {}, (2,), (TILED_STRIDED, TILED_STRIDED, ROW), _ODD),
    Case("tiled", False, {}, (3, 5), _R, ("wide_range",)),
    Case("tiled cut rows", False, {}, (2,), (TILED_STRIDED, TILED_STRIDED, ROW), ("wide_range",)),
]
# every row on both sides: A (fs_spmm, X over columns) and A' (fs_spmm_t, U over rows)
TABLE = [(side, i) for i in range(len(ROWS)) for side in ("A", "At")]


def test_table_reaches_every_plan_on_both_sides():
    """the table is what the GPU tests run: it must name all seven plans on A and on A', each as the default-mode plan of some
    case, with its k admitted by the plan"""
    for side in ("A", "At"):
        default = {ROWS[i].plans[0] for s, i in TABLE if s == side}
        assert default == set(range(1, 8)), (side, sorted(default))
    ks = {k for c in ROWS for k in c.ks}
    assert ks >= {2, 3, 4, 5, 8, 16, 17, 32, 33, 64, 65, 130}, sorted(ks)
    for c in ROWS:
        assert c.copy in COPIES and all(m in ("spmm_kernel", "spmm_wide") for m in c.opts), c
        assert c.plans[2] == ROW, ("strict_order runs the row kernel", c)
        if c.plans[0] == BINNED_K:
            assert all(2 <= k <= 4 for k in c.ks), c
        if c.plans[0] in (LDSX_STRIDED, TILED_STRIDED):
            assert c.ks == (2,), c
        if c.plans[0] == LDSX_COLUMNS:
            assert c.prepared and all(2 <= k <= 16 for k in c.ks), c


# ---- GPU plumbing ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from libfastsparse_amd import capi
    L = capi.lib()
    L.fs_debug_ldsx_orderable.argtypes = [C.c_void_p, C.c_int]
    L.fs_debug_last_spmm_plan.argtypes = []
    L.fs_debug_last_spmm_wide.argtypes = []
    L.fs_debug_tiled_layout.argtypes = [C.c_void_p, C.c_int]
    return L


def _poisoned(shape, fill):
    import torch
    return torch.full(shape, fill, dtype=torch.float64, device="cuda")


def _eq(got, want, what):
    assert E.bits_equal(got, want), f"{what}: {E.first_mismatch(got, want)}"


KMAX = 130
_SETS = {}


def _data(name):
    """three matrices on one pattern -- the exact set ("exact"), its pattern-only form ("pattern") and the pattern with sin values
    ("sin", whose products are not exact: a fused multiply-add shows) -- with the sin panels of the non-exact checks and the
    oracle's results on them: {kind: (Data, X, U, {"A": (A X, |A| |X|), "At": (A' U, |A'| |U|)})}"""
    if name not in _SETS:
        from oracle import pyoracle as O
        d = E.wide_range() if name == "wide_range" else E.wide_range_odd()
        sin_vals = np.sin(np.arange(d.nnz, dtype=np.float64) * 0.37 + 0.2) * np.abs(d.vals)
        out = {}
        for kind, dd in (("exact", d), ("pattern", d.pattern()),
                         ("sin", E.Data(d.name + "_sin", d.nrow, d.ncol, d.rows, d.cols, sin_vals, d.x, d.u, d._xcol))):
            Xs = np.ascontiguousarray(np.sin(np.arange(dd.ncol * KMAX, dtype=np.float64) * 0.7 + 0.1).reshape(dd.ncol, KMAX))
            Us = np.ascontiguousarray(np.sin(np.arange(dd.nrow * KMAX, dtype=np.float64) * 1.3 - 0.4).reshape(dd.nrow, KMAX))
            ref = None
            if kind != "exact":
                v, av = dd.vals, None if dd.vals is None else np.abs(dd.vals)
                ref = dict(
                    A=(O.csr_mul_n(dd.nrow, dd.rp, dd.cols, v, Xs, KMAX), O.csr_mul_n(dd.nrow, dd.rp, dd.cols, av, np.abs(Xs), KMAX)),
                    At=(np.stack([O.coo_tmul(dd.ncol, dd.rows, dd.cols, v, Us[:, j].copy()) for j in range(KMAX)], 1),
                        np.stack([O.coo_tmul(dd.ncol, dd.rows, dd.cols, av, np.abs(Us[:, j])) for j in range(KMAX)], 1)))
            out[kind] = (dd, Xs, Us, ref)
        _SETS[name] = out
    return _SETS[name]


def _build(d, copy):
    from libfastsparse_amd import capi
    with options(**COPIES[copy][0]):
        A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), None if d.vals is None else _d(d.vals))
        A.build_transpose(capi.current_stream())
    return A


def _want_plan(L, A, plan, transposed):
    if isinstance(plan, tuple):
        return plan[0] if L.fs_debug_ldsx_orderable(A.h, int(transposed)) == 1 else plan[1]
    return plan


def _check_copy(A, copy, transposed):
    """the forced copy was kept, by name; a tiled copy has cut rows (a combine pass with the output's stride) exactly when the
    table forces them"""
    from libfastsparse_amd import capi
    want = COPIES[copy][1]
    assert A.kernel_name(transposed) == want, (copy, transposed, A.kernel_name(transposed))
    if want in ("tiled", "lds-staged"):
        layout = capi.lib().fs_debug_tiled_layout(A.h, int(transposed))
        assert layout >= 0 and bool(layout & 1) == (copy == "tiled cut rows"), (copy, transposed, layout)


def _plan_code(A, k, transposed):
    from libfastsparse_amd import capi
    return capi.lib().fs_matrix_spmm_plan(A.h, k, int(transposed))


# ---- the table ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("side,row", TABLE, ids=[f"{s}-{i}-{ROWS[i].copy}{'-prepared' if ROWS[i].prepared else ''}" for s, i in TABLE])
def test_plan_table(hip, side, row):
    from libfastsparse_amd import capi
    L = hip
    case = ROWS[row]
    t = side == "At"
    st = capi.current_stream()
    for set_name in case.sets:
        for kind, (d, Xs, Us, refs) in _data(set_name).items():
            A = _build(d, case.copy)
            _check_copy(A, case.copy, t)
            n_out = d.ncol if t else d.nrow
            if case.prepared:
                with options(**COPIES[case.copy][0], **case.opts):
                    for k in case.ks:
                        A.prepare(k, st, transposed=t)
            for k in case.ks:
                what = (d.name, side, case.copy, case.opts, k)
                if kind != "sin":
                    xe, exact_ref = _d(d.U(k) if t else d.X(k)), (d.Z(k) if t else d.Y(k))
                if kind != "exact":
                    xs = _d(np.ascontiguousarray((Us if t else Xs)[:, :k]))
                    sin_ref, sin_scale = (r[:, :k] for r in refs["At" if t else "A"])
                for mi, mode in enumerate(MODES):
                    with _mode(mode), options(**case.opts):
                        want = _want_plan(L, A, case.plans[mi], t)
                        got_plan = _plan_code(A, k, t)
                        assert got_plan == want, (what, mode, got_plan, want)
                        if kind != "sin":          # exact data: the exact bits in every mode, whole and in parts
                            for fill in (float("nan"), -0.0):
                                Y = _poisoned((n_out, k), fill)
                                L.fs_debug_last_spmm_plan()
                                A.spmm(Y, xe, k, st, transposed=t)
                                assert L.fs_debug_last_spmm_plan() == want, (what, mode, "the launched plan")
                                _eq(Y.cpu().numpy(), exact_ref, (what, mode, fill))
                            for nparts in (1, 3, 7):
                                rows = A.part_rows(nparts, transposed=t, k=k)
                                assert rows[0] == 0 and rows[-1] == n_out and all(a <= b for a, b in zip(rows, rows[1:])), (what, rows)
                                Y = _poisoned((n_out, k), float("nan"))
                                for p in range(nparts):
                                    A.spmm_part(Y, xe, k, p, nparts, st, transposed=t)
                                _eq(Y.cpu().numpy(), exact_ref, (what, mode, nparts, "parts"))
                        if kind == "exact":
                            continue
                        # non-exact data: storage order under strict_order (and wherever the row kernel runs), run-to-run and
                        # part-to-whole identity under reproducible, the row-scaled bar by default
                        Y = _poisoned((n_out, k), float("nan"))
                        A.spmm(Y, xs, k, st, transposed=t)
                        got = Y.cpu().numpy()
                        if mode == "strict_order" or want == ROW:
                            _eq(got, sin_ref, (what, mode, "sin data, storage order"))
                        else:
                            bad = np.abs(got - sin_ref) > 1e-12 * sin_scale
                            assert not bad.any(), (what, mode, "sin data", np.argwhere(bad)[:5])
                        if mode == "reproducible":
                            for _ in range(4):
                                Y2 = _poisoned((n_out, k), -0.0)
                                A.spmm(Y2, xs, k, st, transposed=t)
                                _eq(Y2.cpu().numpy(), got, (what, "reproducible run to run"))
                            for nparts in (3, 7):
                                Y2 = _poisoned((n_out, k), float("nan"))
                                for p in range(nparts):
                                    A.spmm_part(Y2, xs, k, p, nparts, st, transposed=t)
                                _eq(Y2.cpu().numpy(), got, (what, "reproducible in parts", nparts))
            A.close()


# ---- layout branches of the row kernel -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("side", ["A", "At"])
def test_row_kernel_layouts_give_the_bits_of_the_aligned_call(hip, side):
    """spmm_wide = 1: 16-byte loads (spmm_wide_kernel) need an even k and X, Y aligned to 16 bytes.  X or Y 8 bytes off and odd k
    run the narrow kernel (fs_debug_last_spmm_wide says which ran) and must give the bits of the aligned call; on sin data those
    are the oracle's storage-order bits, in every mode"""
    from libfastsparse_amd import capi
    L = hip
    t = side == "At"
    st = capi.current_stream()
    for kind in ("sin", "pattern"):
        d, Xs, Us, refs = _data("wide_range")[kind]
        sin_ref = refs["At" if t else "A"][0]
        n_out, n_in = (d.ncol, d.nrow) if t else (d.nrow, d.ncol)
        A = _build(d, "none")
        for k in (2, 4, 8, 3, 5):
            X = np.ascontiguousarray((Us if t else Xs)[:, :k])
            xbuf = _poisoned((n_in * k + 1,), float("nan"))
            xbuf[1:] = _d(X.reshape(-1))
            for mode in MODES:
                with _mode(mode), options(spmm_kernel=1, spmm_wide=1):
                    assert _plan_code(A, k, t) == ROW
                    Y = _poisoned((n_out, k), float("nan"))
                    L.fs_debug_last_spmm_wide()
                    A.spmm(Y, _d(X), k, st, transposed=t)
                    assert L.fs_debug_last_spmm_wide() == (1 if k % 2 == 0 else 0), (side, k, mode, "16-byte loads where legal")
                    aligned = Y.cpu().numpy()
                    _eq(aligned, sin_ref[:, :k], (d.name, side, k, mode, "aligned"))
                    ybuf = _poisoned((n_out * k + 1,), float("nan"))
                    for xoff, yoff in ((True, False), (False, True), (True, True)):
                        ybuf.fill_(float("nan"))
                        A.spmm(ybuf[1:] if yoff else ybuf[:-1], xbuf[1:] if xoff else _d(X.reshape(-1)), k, st, transposed=t)
                        assert L.fs_debug_last_spmm_wide() == 0, (side, k, mode, xoff, yoff, "misaligned: the narrow kernel")
                        got = (ybuf[1:] if yoff else ybuf[:-1]).cpu().numpy().reshape(n_out, k)
                        _eq(got, aligned, (d.name, side, k, mode, "X off" if xoff else "", "Y off" if yoff else ""))
                        assert np.isnan(ybuf[0 if yoff else -1].item()), "a store outside Y"
        A.close()


# ---- degenerate matrices ----------------------------------------------------------------------------------------------
def _edge_sets():
    rng = np.random.default_rng(31)
    out = []
    x = lambda n, s: np.where(np.random.default_rng(s).uniform(size=n) < 0.5, -1.0, 1.0) * 2.0 ** -2    # noqa: E731
    out.append(E.Data("no_entries", 37, 23, np.zeros(0, int), np.zeros(0, int), np.zeros(0), x(23, 1), x(37, 2), lambda j: x(23, 10 + j)))
    n = 300
    cols = rng.integers(0, n, 200)
    out.append(E.Data("one_row", 1, n, np.zeros(200, int), cols, np.where(rng.uniform(size=200) < 0.5, -1.0, 1.0) *
                      np.ldexp(1.0, rng.integers(0, 20, 200)), x(n, 3), x(1, 4), lambda j: x(n, 20 + j)))
    rows = np.sort(rng.integers(0, n, 250))
    out.append(E.Data("one_column", n, 1, rows, np.zeros(250, int), np.where(rng.uniform(size=250) < 0.5, -1.0, 1.0) *
                      np.ldexp(1.0, rng.integers(0, 20, 250)), x(1, 5), x(n, 6), lambda j: x(1, 30 + j)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("copy", list(COPIES))
def test_degenerate_matrices_on_every_copy(hip, copy):
    """no entries, one row, one column: A and A', k = 2, 3, 5, prepared for k, three modes, NaN-prefilled outputs: exactly +0.0 or
    the exact result.  (A builder may decline a copy for such a matrix: whatever plan serves it must be exact.)"""
    from libfastsparse_amd import capi
    st = capi.current_stream()
    for d in _edge_sets():
        A = _build(d, copy)
        for t in (False, True):
            n_out = d.ncol if t else d.nrow
            for k in (2, 3, 5):
                with options(**COPIES[copy][0]):
                    A.prepare(k, st, transposed=t)
                ref = d.Z(k) if t else d.Y(k)
                inp = _d(d.U(k) if t else d.X(k))
                for mode in MODES:
                    with _mode(mode):
                        assert 1 <= _plan_code(A, k, t) <= 7
                        Y = _poisoned((n_out, k), float("nan"))
                        A.spmm(Y, inp, k, st, transposed=t)
                        _eq(Y.cpu().numpy(), ref, (d.name, copy, t, k, mode))
                        Y = _poisoned((n_out, k), float("nan"))
                        for p in range(3):
                            A.spmm_part(Y, inp, k, p, 3, st, transposed=t)
                        _eq(Y.cpu().numpy(), ref, (d.name, copy, t, k, mode, "3 parts"))
        if d.nnz == 0:
            assert np.all(d.Y(5).view(np.int64) == 0) and np.all(d.Z(5).view(np.int64) == 0)
        A.close()


# ---- the drop-in ------------------------------------------------------------------------------------------------------
def _k_column_entry_points(be, c):
    """the k-column part of _cases.run_case: every reference-named multi-column product, with its name"""
    res = {}
    for name, k in _cases.BIN_SPMM + _cases.BIN_SPMM_VAR:
        if k <= c.kmax:
            res[(f"{name}/k{k}", k)] = lambda name=name, k=k: be.csr_mul_n(c.nrow, c.ncol, c.rows, c.cols, None, c.X(k), k, name)
    bs = c.block_sizes[0]
    for name, k in [("bsbm_A_mul_B2", 2), ("bsbm_A_mul_B4", 4), ("bsbm_A_mul_Bn", 3)]:
        res[(f"{name}/bs{bs}", k)] = lambda name=name, k=k: be.blocked_mul(c.nrow, c.ncol, c.rows, c.cols, None, bs, c.X(k), k, name)
    for k in _cases.VAL_SPMM:
        if k <= c.kmax:
            res[(f"csr_A_mul_Bn/k{k}", k)] = lambda k=k: be.csr_mul_n(c.nrow, c.ncol, c.rows, c.cols, c.vals, c.X(k), k, "csr_A_mul_Bn")
    return res


def _dropin_plans(copy, k, mode, orderable):
    """the plans a prepared handle of the forced copy may run for k (an LDS-staged copy measures sweeps against the row kernel
    for k = 3..16)"""
    if mode == "strict_order":
        return {ROW}
    if copy == "two-pass":
        return {BINNED_K} if k <= 4 else {ROW}
    if mode == "reproducible" and not orderable:
        return {ROW}
    if k == 2:
        return {LDSX_COLUMNS}
    return {LDSX_COLUMNS, ROW} if k <= 16 else {ROW}


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["device", "dropin"])
@pytest.mark.parametrize("copy", ["two-pass", "lds-staged"])
@pytest.mark.parametrize("name", ["wide_range", "wide_range_odd"])
def test_dropin_k_column_entry_points(hip, name, copy, backend):
    """bcsr_A_mul_B2/_B4/_B8/_B8_auto/_Bn/_B32n, bsbm_A_mul_B2/_B4/_Bn, csr_A_mul_Bn with host structs (both backends of
    tests/_cases.run_case), the copy forced around every call: bit for bit against the exact reference, and the plan that served
    each call (fs_debug_last_spmm_plan) is one the copy allows"""
    import _hipbackend as H
    from libfastsparse_amd import capi
    L = hip
    d = _data(name)["exact"][0]
    c = d.case()
    want = _k_column_entry_points(E.ExactBackend(), c)
    be = H.HipDeviceBackend() if backend == "device" else H.HipDropinBackend()
    calls = _k_column_entry_points(be, c)
    with options(**COPIES[copy][0]):
        probe = _build(d, copy)
        orderable = copy == "lds-staged" and L.fs_debug_ldsx_orderable(probe.h, 0) == 1
        probe.close()
        for mode in MODES:
            with _mode(mode):
                for key, f in calls.items():
                    L.fs_debug_last_spmm_plan()
                    got = f()
                    plan = L.fs_debug_last_spmm_plan()
                    assert plan in _dropin_plans(copy, key[1], mode, orderable), (name, copy, backend, mode, key, plan)
                    _eq(got, want[key](), (name, copy, backend, mode, key))
    capi.lib().fs_device_synchronize()


# ---- capture --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("copy,k", [("two-pass", 4), ("two-pass", 2), ("lds-staged", 1), ("lds-staged", 2), ("lds-staged", 8),
                                    ("tiled cut rows", 2)])
def test_products_captured_in_a_graph(hip, copy, k):
    """after prepare, fs_spmm then fs_spmm_t captured on one stream (no parallel branches) and replayed three times on NaN-filled
    outputs: the bits of the eager products, which are the exact ones.  (The LDS-staged copy zeroes its scratch vector on the
    stream: done by a captured hipMemsetAsync, that zeroing went wrong from the second replay on and left rows of Y stale or
    unwritten; products now zero with a kernel, launch_zero.)"""
    import torch
    from libfastsparse_amd import capi
    d = _data("wide_range")["exact"][0]
    A = _build(d, copy)
    if copy == "lds-staged":
        assert capi.lib().fs_debug_tiled_layout(A.h, 0) & 2, "a copy whose chunks share panels: the scratch vector is used"
    st = capi.current_stream()
    opts = dict(spmm_kernel=3) if (copy == "lds-staged" and k > 2) else {}     # one sweep per column for k = 3..16
    with options(**COPIES[copy][0], **opts):
        A.prepare(k, st)
        A.prepare(k, st, transposed=True)
    X, U = _d(d.X(k)), _d(d.U(k))
    want = {"two-pass": BINNED_K, "lds-staged": LDSX_COLUMNS, "tiled cut rows": TILED_STRIDED}[copy] if k > 1 else 0
    with options(**opts):
        assert (_plan_code(A, k, False), _plan_code(A, k, True)) == (want, want), (copy, k)
        Y, Z = _poisoned((d.nrow, k), float("nan")), _poisoned((d.ncol, k), float("nan"))
        A.spmm(Y, X, k, st)
        A.spmm(Z, U, k, st, transposed=True)
        eager_y, eager_z = Y.cpu().numpy(), Z.cpu().numpy()
        _eq(eager_y, d.Y(k), (copy, k, "eager A X"))
        _eq(eager_z, d.Z(k), (copy, k, "eager A' U"))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            s.synchronize()
            with torch.cuda.graph(g, stream=s):
                A.spmm(Y, X, k, capi.current_stream())
                A.spmm(Z, U, k, capi.current_stream(), transposed=True)
    for r in range(3):
        Y.fill_(float("nan"))
        Z.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        _eq(Y.cpu().numpy(), eager_y, (copy, k, "replay", r, "A X"))
        _eq(Z.cpu().numpy(), eager_z, (copy, k, "replay", r, "A' U"))
    del g
    A.close()
