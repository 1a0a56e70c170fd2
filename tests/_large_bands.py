"""The large-band form of the two-pass copy (fs_plan.h: plan_two_pass_geometry's `big`: bands of kBinColsBig = 19 456 columns, panels
of up to kBinRowsBig = 19 456 rows), at the smallest shapes that cross every seam of it: shapes, exact expected values, stand-in
faults, and a runner of GPU cases.

Shapes (both on exactly summable data, tests/_exact.py D2: a = +-odd(1..15) x 2^[-4, 4], x and u integers |.| <= 1023):
  T "thin"   50 000 x 2 000 000, rows 0..149 of 200 entries, every other row one: the builder picks the form itself (fewer than 192
             entries per (band, panel) cell), 103 bands (123 of 16 384), two panels of exactly 19 456 rows; A' has 256 panels, 3 bands
  D "dense"  58 000 x 58 000, H (rows 0..255, 200 distinct columns each) + its mirror + one entry in most other rows: cells of up
             to ~23 000 entries.  The builder would NOT pick the form here; FS_BIN_BIG=1 forces it, and the library reads that
             variable once per process, so D runs in a fresh child: this file as a program,
                 FS_BIN_BIG=1 python tests/_large_bands.py <case> ...
             prints `OK <case>` (then `TIME <case> <seconds>`) per case, `FAIL <case>: <message>` at the first case that raises,
             and exits non-zero there.  tests/test_gpu_two_pass_large_bands.py starts it once and asserts case by case.
tests/test_large_bands_shapes.py holds the shapes to what is said here, on the CPU, from tests/_plan_model.py."""
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)

import _exact as E  # noqa: E402
import _plan_model as M  # noqa: E402
from _gpu import PRODUCT_MODES as MODES, mode_options as _mode, options, to_device as _d  # noqa: E402

BIG, SMALL = M.K_BIN_COLS_BIG, M.K_BIN_COLS          # 19 456 and 16 384: band widths, and the tallest panels, of the two forms
BINNED_COLS = 3                                      # fs_matrix_spmm_plan: one single-vector two-pass sweep per column
NAN_COL = 18_000                                     # D: a column of band 0 whose local id is above 16 383
K = 3


# ---- shapes ---------------------------------------------------------------------------------------------------------
def _d2(name, nrow, ncol, rows, cols, seed):
    """D2 values and vectors on a pattern given in row-major order"""
    rng = np.random.default_rng(seed)
    vals = E._signs(rng, rows.size) * np.ldexp(E._odd(rng, rows.size, 15), rng.integers(-4, 5, rows.size))
    x = rng.integers(-1023, 1024, ncol).astype(np.float64)
    u = rng.integers(-1023, 1024, nrow).astype(np.float64)
    xcol = lambda j: np.random.default_rng(seed * 1000 + j).integers(-1023, 1024, ncol).astype(np.float64)   # noqa: E731
    return E.Data(name, nrow, ncol, rows, cols, vals, x, u, xcol)


def thin(seed=31):
    nrow, ncol = 50_000, 2_000_000
    rng = np.random.default_rng(seed)
    lens = np.ones(nrow, np.int64)
    lens[:150] = 200
    rows, cols = E._coo(lens, ncol, rng)
    return _d2("thin", nrow, ncol, rows, cols, seed + 1)


def dense(seed=37):
    n = 58_000
    rng = np.random.default_rng(seed)
    hr = np.repeat(np.arange(256), 200)
    hc = np.concatenate([rng.choice(n, 200, replace=False) for _ in range(256)])
    sr = np.arange(256, n)
    sc = rng.integers(0, n, sr.size)
    keep = rng.uniform(size=sr.size) >= 0.05
    sc[20_000 - 256], keep[20_000 - 256] = n - 1, True          # the last column of the last band is referenced (row 20 000)
    sc[30_000 - 256], keep[30_000 - 256] = NAN_COL, True        # and so is NAN_COL, from a row that holds nothing else of H
    key = np.unique(np.concatenate([hr * n + hc, hc * n + hr, sr[keep] * n + sc[keep]]).astype(np.int64))   # row-major, no duplicates
    return _d2("dense", n, n, key // n, key % n, seed + 1)


def heavy():
    """config 5's own combination: long rows out of the two-pass copy, the rest on the large-band form (test_long_rows_are_exact's set)"""
    return E.long_rows(profile="heavy", nrow=150_000, ncol=200_000, seed=8)


SHAPES = {"T": thin, "D": dense}
_DATA = {}


def data(shape, valued=True):
    """the shape's Data, built once per process; valued=False: the same pattern without values"""
    if shape not in _DATA:
        d = SHAPES[shape]()
        _DATA[shape] = {True: d, False: d.pattern()}
    return _DATA[shape][valued]


def transposed(d):
    """A' as a Data of its own (row-major in the columns of A), x and u swapped; made once per Data"""
    if "t" not in d._cache:
        order = np.lexsort((d.rows, d.cols))
        d._cache["t"] = E.Data(d.name + "_t", d.ncol, d.nrow, d.cols[order], d.rows[order], None if d.vals is None else d.vals[order],
                               d.u, d.x, d.ucol)
    return d._cache["t"]


def side(shape, valued, t):
    """A (t = 0) or A' (t = 1) of a shape as a Data whose y() is the product of that side"""
    d = data(shape, valued)
    return transposed(d) if t else d


# ---- the layout the planner gives a side (tests/_plan_model.py) -------------------------------------------------------
def bin_env():
    """FS_BIN_BIG as build_binned_impl reads it: -1 unset (the builder decides), 0 never, otherwise always"""
    return int(os.environ.get("FS_BIN_BIG") or -1)


def layout(d, big_env, slots=256):
    """what build_binned_impl lays out for d's CSR with `slots` pass-2 workgroups: geometry, panels, local ids of every entry"""
    vp, cut = M.virtual_rows(d.rp, 256)
    assert not cut, "a row above 256 entries: cut rows are not what these shapes are about"
    g = M.plan_two_pass_geometry(d.nrow, d.ncol, d.nnz, 1, 0, big_env)
    panel_row = np.asarray(M.plan_two_pass_panels(vp, d.nrow, d.nnz, g["R"], slots, float(os.environ.get("FS_BIN_FILL") or 80) / 100.0,
                                                  int(os.environ.get("FS_BIN_MIN_PANELS") or 1), 1), np.int64)
    bc = g["bcols"]
    B, P = -(-d.ncol // bc), panel_row.size - 1
    rows, cols = d.rows.astype(np.int64), d.cols.astype(np.int64)
    panel = np.searchsorted(panel_row[:-1], rows, side="right") - 1
    cells = np.bincount(panel * B + cols // bc, minlength=P * B)
    return dict(big=g["big"], bcols=bc, B=B, B_small=-(-d.ncol // SMALL), P=P, panel_row=panel_row, panel_rows=np.diff(panel_row),
                band=cols // bc, lcol=cols % bc, panel=panel, lrow=rows - panel_row[panel], cells=cells, last_band=d.ncol - (B - 1) * bc)


# ---- stand-in faults (numpy): what a subtly wrong kernel of this form would compute ---------------------------------
def _sum(d, xi):
    """A x with x gathered at the (possibly wrong) columns xi; D2 data: |a x| < 2^18 in multiples of 2^-4, rows of at most a few
    thousand entries, so the fp64 sums are exact in any order"""
    t = d.x[xi] if d.vals is None else d.vals * d.x[xi]
    return np.bincount(d.rows, weights=t, minlength=d.nrow)


def faults(d, lay, prefill=np.nan):
    """{name: y} of three faults on the large-band layout `lay` of d"""
    assert lay["bcols"] == BIG
    out = {"local column id modulo 16 384": _sum(d, lay["band"] * BIG + lay["lcol"] % SMALL),
           "band start b * 16 384": _sum(d, lay["band"] * SMALL + lay["lcol"])}
    y = _sum(d, d.cols)
    local = np.arange(d.nrow) - np.repeat(lay["panel_row"][:-1], lay["panel_rows"])
    y[local >= SMALL] = prefill
    out["rows from local row 16 384 on left at their prefill"] = y
    return out


# ---- GPU plumbing -----------------------------------------------------------------------------------------------------
def _lib():
    from libfastsparse_amd import capi
    L = capi.lib()
    L.fs_debug_two_pass_layout.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]
    L.fs_debug_two_pass_rows8.restype = C.c_longlong
    L.fs_debug_two_pass_rows8.argtypes = [C.c_void_p, C.c_int]
    L.fs_debug_long_rows.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.fs_debug_last_spmm_plan.argtypes = []
    return L


def _poisoned(shape, fill):
    import torch
    return torch.full(shape, fill, dtype=torch.float64, device="cuda")


def _eq(got, want, what):
    assert E.bits_equal(got, want), f"{what}: {E.first_mismatch(got, want)}"


def _ncu():
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return ncu if ncu > 0 else 256


def assert_form(A, d, sides=(0, 1), long_rows=False):
    """the large-band form ran, on the sides named: by name, by the band and panel counts the planner gives for this device, and by
    the two-byte row ids the form keeps.  (A copy with long rows is laid out from the CSR without them: its bands are checked, its
    panels are not predicted here.)"""
    L = _lib()
    env = bin_env()
    assert env != 0, "FS_BIN_BIG=0 in the environment switches the form under test off"
    for t in sides:
        ncol = d.nrow if t else d.ncol
        assert A.kernel_name(bool(t)) == "two-pass", (d.name, t, A.kernel_name(bool(t)))
        with _mode("strict_order"):
            assert A.kernel_name(bool(t)) == "stream", (d.name, t)
        out = (C.c_ulonglong * 8)()
        assert L.fs_debug_two_pass_layout(A.h, t, out) == 0
        B, P = int(out[6]), int(out[7])
        assert B == -(-ncol // BIG) and B != -(-ncol // SMALL), (d.name, t, B, "bands of 19 456 columns")
        assert L.fs_debug_two_pass_rows8(A.h, t) == -1, (d.name, t, "two-byte row ids")
        if not long_rows:
            lay = layout(transposed(d) if t else d, env, _ncu())
            assert lay["big"] == 1 and (B, P) == (lay["B"], lay["P"]), (d.name, t, (B, P), (lay["B"], lay["P"]))


_COPIES = {}


def copy_of(shape, valued):
    """the shape's copy with its A', built once per process and checked to be of the form before anything is run on it"""
    from libfastsparse_amd import capi
    key = (shape, valued)
    if key not in _COPIES:
        d = data(shape, valued)
        with options(binning=2, ldsx=0, tiling=0, long_rows=0):
            A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), None if d.vals is None else _d(d.vals))
            A.build_transpose(capi.current_stream())
        assert_form(A, d)
        _COPIES[key] = A
    return _COPIES[key], data(shape, valued)


def _spmv(A, v, n, t, fill=float("nan")):
    from libfastsparse_amd import capi
    out = _poisoned((n,), fill)
    A.spmv(out, v, capi.current_stream(), transposed=bool(t))
    return out.cpu().numpy()


# ---- the cases --------------------------------------------------------------------------------------------------------
def case_form(shape, valued):
    """1. the form ran (copy_of asserts it for every case; this one is the report of it)"""
    copy_of(shape, valued)


def case_products(shape, valued):
    """2. A x and A' u in three modes, y prefilled with NaN and with -0.0: the exact sums, +0.0 in empty rows.  "reproducible" is
    spmv_reduce_ordered_kernel<false, kBinRowsBig>; strict_order leaves the copy for the chunk-streaming kernel."""
    A, d = copy_of(shape, valued)
    refs = (d.y(), d.z())
    assert (refs[0] == 0).any()
    vs = (_d(d.x), _d(d.u))
    for mode in MODES:
        with _mode(mode):
            for t in (0, 1):
                assert A.kernel_name(bool(t)) == ("stream" if mode == "strict_order" else "two-pass")
                for fill in (float("nan"), -0.0):
                    _eq(_spmv(A, vs[t], refs[t].size, t, fill), refs[t], (shape, valued, mode, fill, "A' u" if t else "A x"))


def case_plain_loads(shape, valued):
    """3. bin_flags = 256 at product time: pass 2 with plain product loads, spmv_reduce_kernel<false, kBinRowsBig, false>"""
    A, d = copy_of(shape, valued)
    with options(bin_flags=256):
        for t, v, ref in ((0, d.x, d.y()), (1, d.u, d.z())):
            assert A.kernel_name(bool(t)) == "two-pass"
            for fill in (float("nan"), -0.0):
                _eq(_spmv(A, _d(v), ref.size, t, fill), ref, (shape, valued, "plain loads", fill, t))


def case_parts(shape, valued):
    """4. the product in 3 and in 4 parts: part_rows monotone from 0 to nrow, after part p the rows below rows[p + 1] final, all
    parts together the exact bits.  On these shapes a copy has at most 256 panels -- one generation of resident workgroups on an
    MI355X -- so the parts may not really be cut (rows = 0, nrow, nrow, ...): what is checked is that the large-band kernels are
    reached through the part launcher with the right ranges.  The real cut of this form stays with the full-size config-5 test."""
    from libfastsparse_amd import capi
    A, d = copy_of(shape, valued)
    st = capi.current_stream()
    for mode in MODES:
        with _mode(mode):
            for t, v, ref in ((0, d.x, d.y()), (1, d.u, d.z())):
                vd = _d(v)
                for nparts in (3, 4):
                    rows = A.part_rows(nparts, transposed=bool(t))
                    assert rows[0] == 0 and rows[-1] == ref.size and all(a <= b for a, b in zip(rows, rows[1:])), (shape, t, rows)
                    y = _poisoned((ref.size,), float("nan"))
                    for p in range(nparts):
                        A.spmv_part(y, vd, p, nparts, st, transposed=bool(t))
                        _eq(y[:rows[p + 1]].cpu().numpy(), ref[:rows[p + 1]], (shape, valued, mode, t, nparts, "after part", p))
                    _eq(y.cpu().numpy(), ref, (shape, valued, mode, t, nparts, "parts"))


def case_host(shape, valued):
    """5. host vectors: x up by ranges of bands (spmv_expand_kernel<V, 4, false, true, kBinColsBig> from launch_expand_groups), y
    down by ranges of panels; fs_debug_last_host_path == 1 says that this way was taken"""
    from libfastsparse_amd import capi
    A, d = copy_of(shape, valued)
    with _mode("default"):                            # (fixed-order sums take the other way: copy, product, copy)
        for t, v, ref in ((0, d.x, d.y()), (1, d.u, d.z())):
            for fill in (np.nan, -0.0):
                yh = np.full(ref.size, fill)
                A.spmv_host(yh, v, transposed=bool(t))
                assert capi.lib().fs_debug_last_host_path() == 1, (shape, t, capi.lib().fs_debug_last_host_path())
                _eq(yh, ref, (shape, valued, "host vectors", fill, t))


def case_strided(shape, valued):
    """6. k = 3 columns under spmm_kernel = 3: one single-vector sweep per column with xs = ys = 3 through the large-band kernels"""
    from libfastsparse_amd import capi
    A, d = copy_of(shape, valued)
    L = _lib()
    st = capi.current_stream()
    for mode in ("default", "reproducible"):
        with options(spmm_kernel=3), _mode(mode):
            for t, X, ref in ((0, d.X(K), d.Y(K)), (1, d.U(K), d.Z(K))):
                assert L.fs_matrix_spmm_plan(A.h, K, t) == BINNED_COLS, (shape, t, L.fs_matrix_spmm_plan(A.h, K, t))
                for fill in (float("nan"), -0.0):
                    Y = _poisoned(ref.shape, fill)
                    L.fs_debug_last_spmm_plan()
                    A.spmm(Y, _d(X), K, st, transposed=bool(t))
                    assert L.fs_debug_last_spmm_plan() == BINNED_COLS, (shape, t, "the launched plan")
                    _eq(Y.cpu().numpy(), ref, (shape, valued, mode, "k = 3", fill, t))
    assert capi.lib().fs_get_option(b"spmm_kernel") != 3


def case_non_finite(shape, valued):
    """7. NaN in a column of band 0 with a local id above 16 383, +inf in the last column of the last band: exactly the rows that
    reference them are NaN / inf as IEEE gives, every other row keeps its exact bits -- the padding entries point at slot 19 456 of
    the band and stay silent"""
    A, d = copy_of(shape, valued)
    lay = layout(d, 1)
    inf_col = d.ncol - 1
    assert SMALL <= NAN_COL < BIG and (inf_col // BIG, inf_col % BIG) == (lay["B"] - 1, lay["last_band"] - 1)
    x = d.x.copy()
    x[NAN_COL], x[inf_col] = np.nan, np.inf
    hit_nan, hit_inf = np.zeros(d.nrow, bool), np.zeros(d.nrow, bool)
    hit_nan[d.rows[d.cols == NAN_COL]] = True
    hit_inf[d.rows[d.cols == inf_col]] = True
    assert hit_nan.sum() > 0 and (hit_inf & ~hit_nan).sum() > 0 and (hit_nan | hit_inf).sum() < 50
    with np.errstate(invalid="ignore"):
        ieee = np.bincount(d.rows, weights=x[d.cols] if d.vals is None else d.vals * x[d.cols], minlength=d.nrow)
    bad, only_inf = hit_nan | hit_inf, hit_inf & ~hit_nan
    assert np.all(np.isnan(ieee[hit_nan])) and np.all(np.isinf(ieee[only_inf]))
    ref = d.y()
    for mode in ("default", "reproducible"):
        with _mode(mode):
            assert A.kernel_name() == "two-pass"
            for fill in (float("nan"), -0.0):
                got = _spmv(A, _d(x), d.nrow, 0, fill)
                assert np.array_equal(~np.isfinite(got), bad), (mode, fill, np.flatnonzero(~np.isfinite(got) != bad)[:5])
                assert np.all(np.isnan(got[hit_nan])), (mode, fill)
                assert np.array_equal(got[only_inf], ieee[only_inf]), (mode, fill, "inf rows carry the sign IEEE gives")
                _eq(got[~bad], ref[~bad], (mode, fill, "finite rows beside non-finite x"))


def case_rounding(shape, valued):
    """8. data that round (|a|, |x| <= 1): the default product within the project's bar of 1e-12 x row length of the strict_order
    product, under "reproducible" two products with identical bits within the same bar; the same for A' u with column counts"""
    from libfastsparse_amd import capi
    assert valued
    d = data(shape, True)
    vals = np.random.default_rng(99).uniform(-1.0, 1.0, d.nnz)
    with options(binning=2, ldsx=0, tiling=0, long_rows=0):
        A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), _d(vals))
        A.build_transpose(capi.current_stream())
    assert_form(A, d)
    x, u = np.sin(7.0 * np.arange(d.ncol) + 0.3), np.sin(11.0 * np.arange(d.nrow) - 0.2)
    lens = (np.diff(d.rp), np.bincount(d.cols, minlength=d.ncol))
    for t, v in ((0, x), (1, u)):
        vd, n = _d(v), lens[t].size
        with _mode("strict_order"):
            assert A.kernel_name(bool(t)) == "stream"
            ref = _spmv(A, vd, n, t)
        assert A.kernel_name(bool(t)) == "two-pass"
        y = _spmv(A, vd, n, t)
        worst = float(np.max(np.abs(y - ref) - 1e-12 * lens[t]))
        assert np.all(np.abs(y - ref) <= 1e-12 * lens[t]), (t, "default", worst)
        with _mode("reproducible"):
            assert A.kernel_name(bool(t)) == "two-pass"
            y1, y2 = _spmv(A, vd, n, t), _spmv(A, vd, n, t, -0.0)
        _eq(y2, y1, (t, "reproducible, run to run"))
        assert np.all(np.abs(y1 - ref) <= 1e-12 * lens[t]), (t, "reproducible", float(np.max(np.abs(y1 - ref))))
    A.close()


def case_long_rows():
    """the long-row path joined to the large-band copy: rows of >= 32 entries leave the two-pass copy (fs_debug_long_rows), the rest
    sits on 11 bands of 19 456 columns (13 of 16 384); A x exact in three modes, in 3 parts and with host vectors"""
    from libfastsparse_amd import capi
    L = _lib()
    d = heavy()
    ref = d.y()
    with options(binning=2, long_rows=2, long_min_len=32):
        A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), _d(d.vals))
    info = (C.c_int64 * 2)()
    assert L.fs_debug_long_rows(A.h, 0, info) == 0 and info[0] > 0, info[0]
    assert_form(A, d, sides=(0,), long_rows=True)
    out = (C.c_ulonglong * 8)()
    assert L.fs_debug_two_pass_layout(A.h, 0, out) == 0 and int(out[6]) == 11 and -(-d.ncol // SMALL) == 13, int(out[6])
    st = capi.current_stream()
    xd = _d(d.x)
    for mode in MODES:
        with _mode(mode):
            assert A.kernel_name() == ("stream" if mode == "strict_order" else "two-pass")
            for fill in (float("nan"), -0.0):
                _eq(_spmv(A, xd, d.nrow, 0, fill), ref, ("long rows", mode, fill))
            y = _poisoned((d.nrow,), float("nan"))
            for part in range(3):
                A.spmv_part(y, xd, part, 3, st)
            _eq(y.cpu().numpy(), ref, ("long rows", mode, "in 3 parts"))
            yh = np.full(d.nrow, np.nan)
            A.spmv_host(yh, d.x)
            _eq(yh, ref, ("long rows", mode, "host vectors"))
    A.close()


PER_COPY = {"form": case_form, "products": case_products, "plain_loads": case_plain_loads, "parts": case_parts, "host": case_host,
            "strided": case_strided}


def _cases(shape):
    out = {}
    for valued in (True, False):
        for name, f in PER_COPY.items():
            out[f"{shape}-{'valued' if valued else 'pattern'}-{name}"] = (f, (shape, valued))
    return out


T_CASES = _cases("T")                                 # in process: the builder picks the form
D_CASES = _cases("D")                                 # in a child with FS_BIN_BIG=1
D_CASES.update({"D-valued-non_finite": (case_non_finite, ("D", True)), "D-pattern-non_finite": (case_non_finite, ("D", False)),
                "D-valued-rounding": (case_rounding, ("D", True)), "long_rows": (case_long_rows, ())})
CASES = dict(T_CASES, **D_CASES)


def run(name):
    f, args = CASES[name]
    f(*args)


def main(argv):
    import torch  # (before the library, like the suite's fixtures: one HIP runtime per process, the one torch brings)
    assert torch.cuda.is_available(), "the large-band cases need a GPU"
    for name in argv or list(D_CASES):
        t0 = time.time()
        try:
            run(name)
        except BaseException as e:                    # the first case that raises ends the run: nothing after a failure is started
            msg = " ".join(f"{type(e).__name__}: {e}".split())
            print(f"FAIL {name}: {msg[:2000]}", flush=True)
            return 1
        print(f"OK {name}", flush=True)
        print(f"TIME {name} {time.time() - t0:.2f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
