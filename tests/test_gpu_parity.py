"""GPU parity tests: the HIP path, called through the C-ABI, against the oracle and the reference goldens.

Bars (SURVEY.md 8a notes N1/N2, BASELINE.json north_star):
  * integer-valued x: bit-exact, always (any summation order is exact below 2^53);
  * strict_order=1: bit-exact for arbitrary x (thread-per-row sums in storage order, no FMA);
  * default mode, arbitrary x: |y_gpu - y_ref| <= 1e-12 * sum_j |a_ij||x_j| per element.
"""
import os

import numpy as np
import pytest

import _cases
import _kats
import _synth as S
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-12
CASES = _cases.all_cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import _hipbackend as H
    return H


VALUED = ("sdm_A_mul_B", "sdm_At_mul_B", "csr_A_mul_B", "csr_A_mul_Bn", "bsdm_A_mul_B")


_SCALES = {}


def _scales(name):
    """sum_j |a_ij||x_j| of every output element of a case: the same products on |A|, |x| through the oracle (cached per case)"""
    if name not in _SCALES:
        _SCALES[name] = _cases.run_case(_cases.OracleBackend(), BY_NAME[name], absolute=True)
    return _SCALES[name]


def _check(out, gold, name, exact):
    """exact: every output bit for bit.  Otherwise: pattern-only products of integer-valued x bit for bit
    (order-independent), everything else ROW-SCALED: |y - y_ref| <= TOL * sum_j |a_ij||x_j| per
    element, the bound the full-size tests use (test_gpu_fullsize.py) -- an output whose terms are all zero must be exact."""
    scales = None
    for k, v in out.items():
        g = gold[k.replace("/", "|")]
        assert v.shape == g.shape, (name, k)
        if k.startswith("bsbm_cg"):
            # iterative consumer: device reductions are tree sums, so iterates follow the CPU's to
            # rounding; the stopping iteration may move by one when ||r|| lands on the threshold
            if k.endswith("/iter"):
                assert abs(v[0] - g[0]) <= 1, (name, k, v, g)
            else:
                assert np.max(np.abs(v - g)) <= 1e-5 * max(1e-300, float(np.max(np.abs(g)))), (name, k)
            continue
        if exact or (k.endswith("/int") and k.split("/")[0] not in VALUED):
            assert np.array_equal(v.view(np.int64), g.view(np.int64)), \
                f"{name}:{k} not bit-exact (max diff {np.max(np.abs(v - g))})"
        else:
            if scales is None:
                scales = _scales(name)
            sc = scales[k]
            assert sc.shape == g.shape, (name, k)
            excess = np.abs(v - g) - TOL * sc
            assert np.all(excess <= 0), \
                f"{name}:{k} off by {np.max(np.abs(v - g))}, {np.max(excess)} beyond the row-scaled bound (worst scale {sc.flat[int(np.argmax(excess))]})"


@pytest.mark.parametrize("backend", ["device", "dropin"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_all_entry_points_vs_reference_golden(hip, backend, case):
    from libfastsparse_amd import capi
    capi.set_option("strict_order", 0)
    be = hip.HipDeviceBackend() if backend == "device" else hip.HipDropinBackend()
    gold = np.load(os.path.join(S.GOLDEN, case.name + ".npz"))
    out = _cases.run_case(be, case)
    assert set(k.replace("/", "|") for k in out) == set(gold.files)
    _check(out, gold, case.name, exact=False)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_strict_order_is_bit_exact(hip, case):
    from libfastsparse_amd import capi
    capi.set_option("strict_order", 1)
    try:
        gold = np.load(os.path.join(S.GOLDEN, case.name + ".npz"))
        out = _cases.run_case(hip.HipDeviceBackend(), case)
        _check(out, gold, case.name, exact=True)
    finally:
        capi.set_option("strict_order", 0)


@pytest.mark.parametrize("backend", ["device", "dropin"])
def test_reference_kats(hip, backend):
    be = hip.HipDeviceBackend() if backend == "device" else hip.HipDropinBackend()
    _kats.check_kats(be, BY_NAME)


@pytest.mark.parametrize("kernel", [1, 2, 3])
def test_kernel_variants_agree(hip, kernel):
    """streaming kernel (nt / cached loads) and the lanes-per-row kernel: same bits for the pattern-only
    matrix with integer x, 1e-12 for the valued one"""
    from libfastsparse_amd import capi
    capi.set_option("spmv_kernel", kernel)
    try:
        be = hip.HipDeviceBackend()
        for name in ("syn_u16_2048", "syn_long_800x5000", "syn_empty_1500x900"):
            c = BY_NAME[name]
            gold = np.load(os.path.join(S.GOLDEN, name + ".npz"))
            y = be.csr_mul(c.nrow, c.ncol, c.rows, c.cols, None, c.xs["int"])
            assert np.array_equal(y, gold["bcsr_A_mul_B|int"])
            rp, cc, vv = O.coo_to_csr(c.nrow, c.rows, c.cols, c.vals)
            for tag in ("int", "bench"):
                y = be.csr_mul(c.nrow, c.ncol, c.rows, c.cols, c.vals, c.xs[tag])
                g = gold["csr_A_mul_B|" + tag]
                scale = O.csr_abs_scale(c.nrow, rp, cc, vv, c.xs[tag])       # |y - y_ref| <= 1e-12 sum_j |a_ij||x_j|
                assert np.all(np.abs(y - g) <= TOL * scale), (name, tag, float(np.max(np.abs(y - g) - TOL * scale)))
    finally:
        capi.set_option("spmv_kernel", 0)


@pytest.mark.parametrize("backend", ["device", "dropin"])
def test_csr_transposed_product(hip, backend):
    """CSR At_mul_B (SURVEY note N3) = sdm_At_mul_B semantics on the same entries, y overwritten"""
    be = hip.HipDeviceBackend() if backend == "device" else hip.HipDropinBackend()
    for name in ("fix_sdm_100x50", "syn_empty_1500x900", "syn_long_800x5000"):
        c = BY_NAME[name]
        for vals in (c.vals, None):
            for tag in ("int", "bench"):
                xt = c.xt(tag)
                # oracle order: column sums in CSR (row-major) entry order
                rp, cc, vv = O.coo_to_csr(c.nrow, c.rows, c.cols, vals)
                rows_sorted = np.repeat(np.arange(c.nrow, dtype=np.int32), np.diff(rp))
                ref = O.coo_tmul(c.ncol, rows_sorted, cc, vv, xt)
                y = be.transposed_csr_mul(c.nrow, c.ncol, c.rows, c.cols, vals, xt)
                if tag == "int" and vals is None:
                    assert np.array_equal(y, ref), (name, tag)
                else:       # row-scaled: the same column sums on |A|, |x|
                    scale = O.coo_tmul(c.ncol, rows_sorted, cc, None if vv is None else np.abs(vv), np.abs(xt))
                    assert np.all(np.abs(y - ref) <= TOL * scale), (name, tag, float(np.max(np.abs(y - ref) - TOL * scale)))


@pytest.mark.parametrize("geometry", [(64, 128), (7, 33), (2048, 4096), (0, 0)])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_tiled_kernel_vs_reference_golden(hip, case, geometry):
    """the L2-tiled (row panel x column band) kernel, forced on with small panels/bands so that every case
    spans many tiles; (0, 0) = automatic geometry"""
    from libfastsparse_amd import capi
    capi.set_option("tiling", 2)
    capi.set_option("tile_rows", geometry[0])
    capi.set_option("tile_cols", geometry[1])
    try:
        gold = np.load(os.path.join(S.GOLDEN, case.name + ".npz"))
        out = _cases.run_case(hip.HipDeviceBackend(), case, light=True)
        _check(out, gold, case.name, exact=False)
        # reproducible run to run: the band-major order is fixed
        out2 = _cases.run_case(hip.HipDeviceBackend(), case, light=True)
        for k in out:
            assert np.array_equal(out[k].view(np.int64), out2[k].view(np.int64)), k
    finally:
        capi.set_option("tiling", 1)
        capi.set_option("tile_rows", 0)
        capi.set_option("tile_cols", 0)


@pytest.mark.parametrize("split", [3, 37, 1000])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_tiled_kernel_with_cut_rows(hip, case, split):
    """rows longer than `split` entries are cut into virtual rows (nnz-balanced panels, per-row combine pass):
    same results as the reference within the fp64 bar, bit-exact for pattern-only integer products, and
    reproducible run to run"""
    from libfastsparse_amd import capi
    capi.set_option("tiling", 2)
    capi.set_option("tile_rows", 64)
    capi.set_option("tile_cols", 128)
    capi.set_option("tile_split", split)
    try:
        gold = np.load(os.path.join(S.GOLDEN, case.name + ".npz"))
        out = _cases.run_case(hip.HipDeviceBackend(), case, light=True)
        _check(out, gold, case.name, exact=False)
        out2 = _cases.run_case(hip.HipDeviceBackend(), case, light=True)
        for k in out:
            assert np.array_equal(out[k].view(np.int64), out2[k].view(np.int64)), k
    finally:
        capi.set_option("tiling", 1)
        capi.set_option("tile_rows", 0)
        capi.set_option("tile_cols", 0)
        capi.set_option("tile_split", 0)


def test_edge_shapes(hip):
    """empty matrix, single row/column, all rows empty, row longer than several chunks, k not a power of two"""
    be = hip.HipDeviceBackend()
    i32 = np.int32
    # nnz == 0
    y = be.coo_mul(5, 3, np.empty(0, i32), np.empty(0, i32), None, np.ones(3))
    assert np.array_equal(y, np.zeros(5))
    # 1 x 1
    y = be.coo_mul(1, 1, np.array([0], i32), np.array([0], i32), np.array([2.5]), np.array([4.0]))
    assert y[0] == 10.0
    # one row spanning 5 chunks + trailing empty rows
    n = 5 * 2048 + 77
    rows = np.full(n, 2, i32)
    cols = (np.arange(n) % 1000).astype(i32)
    vals = S.x_sin(n, 3.0, 0.1)
    x = S.x_int(5, 1000)
    rp, cc, vv = O.coo_to_csr(7, rows, cols, vals)
    y = be.coo_mul(7, 1000, rows, cols, vals, x)
    ref = O.csr_mul(7, rp, cc, vv, x)
    assert np.max(np.abs(y - ref)) <= TOL * np.sum(np.abs(vals) * np.abs(x[cols]))
    assert np.array_equal(y[[0, 1, 3, 4, 5, 6]], np.zeros(6))
    yb = be.coo_mul(7, 1000, rows, cols, None, x)
    assert np.array_equal(yb, O.csr_mul(7, rp, cc, None, x))      # integer x: exact
    # odd k and k > 64
    c = BY_NAME["syn_dup_1024"]
    rp, cc, vv = O.coo_to_csr(c.nrow, c.rows, c.cols, c.vals)
    for k in (1, 3, 7, 33, 70):
        X = S.X_sin(c.ncol, k)
        Y = be.csr_mul_n(c.nrow, c.ncol, c.rows, c.cols, c.vals, X, k, "csr_A_mul_Bn")
        ref = O.csr_mul_n(c.nrow, rp, cc, vv, X, k)
        if k == 1:   # k = 1 is the SpMV kernel: rows that cross a chunk are sums of partial sums
            assert np.max(np.abs(Y - ref)) <= TOL * max(1.0, np.max(np.abs(ref)))
        else:        # the multi-column kernel adds every row's terms in storage order
            assert np.array_equal(Y, ref), k


def test_y_is_overwritten(hip):
    """outputs are pre-poisoned with -1 by the backends (as test_sparse.c:460 does): empty rows must be +0"""
    be = hip.HipDropinBackend()
    c = BY_NAME["syn_empty_1500x900"]
    y = be.csr_mul(c.nrow, c.ncol, c.rows, c.cols, c.vals, c.xs["bench"])
    rp, _, _ = O.coo_to_csr(c.nrow, c.rows, c.cols, c.vals)
    empty = np.diff(rp) == 0
    assert empty.any() and np.all(y[empty] == 0.0) and not np.signbit(y[empty]).any()


def test_device_format_builders_match_oracle(hip):
    """device COO->CSR (stable) and device transpose produce the arrays the host builders produce"""
    from libfastsparse_amd import capi
    import torch
    c = BY_NAME["syn_dup_1024"]
    d = lambda a: torch.from_numpy(a).cuda()
    m = capi.Matrix.from_coo(c.nrow, c.ncol, d(c.rows), d(c.cols), d(c.vals))
    rp, cc, vv = O.coo_to_csr(c.nrow, c.rows, c.cols, c.vals)
    grp, gcc, gvv = m.download()
    assert np.array_equal(grp, rp) and np.array_equal(gcc, cc) and np.array_equal(gvv, vv)
    m.build_transpose(capi.current_stream())
    rows_sorted = np.repeat(np.arange(c.nrow, dtype=np.int32), np.diff(rp))
    trp, tcc, tvv = O.coo_to_csr(c.ncol, cc, rows_sorted, vv)
    grp, gcc, gvv = m.download(transposed=True)
    assert np.array_equal(grp, trp) and np.array_equal(gcc, tcc) and np.array_equal(gvv, tvv)


def test_synthetic_generator_matches_cpu_twin(hip):
    """bench inputs: the device generator and oracle/fs_synth.c produce identical arrays"""
    from libfastsparse_amd import capi
    from oracle import pysynth
    rp, cc, vv = capi.synth_uniform(5000, 77777, 16, 0x5EED0002, row_offset=123)
    hrp, hcc, hvv = pysynth.uniform(5000, 77777, 16, 0x5EED0002, row_offset=123)
    assert np.array_equal(rp.cpu().numpy(), hrp) and np.array_equal(cc.cpu().numpy(), hcc)
    assert np.array_equal(vv.cpu().numpy(), hvv)
    rp, cc, vv = capi.synth_powerlaw(20000, 50000, 2.3, 100000, 0x5EED0005, row_offset=7)
    hrp, hcc, hvv = pysynth.powerlaw(20000, 50000, 2.3, 100000, 0x5EED0005, row_offset=7)
    assert np.array_equal(rp.cpu().numpy(), hrp) and np.array_equal(cc.cpu().numpy(), hcc)
    assert np.array_equal(vv.cpu().numpy(), hvv)


def test_c_bench_driver_config1(hip):
    """BASELINE config 1 (plumbing): the label-compatible C driver runs on both bundled fixtures, host and
    device vectors, and prints every section of the reference's bench plus [csr-f64]"""
    import subprocess
    from libfastsparse_amd import _build
    exe = _build.build_c_bench()
    labels = ["unsorted", "sort", "block", "2xblock", "2xblock*", "cg", "cg2", "csr", "csr2", "cg2-csr", "cg4-csr",
              "cg8-csr", "cg8a-csr", "cg8*-csr", "cg8**-csr", "4xblock", "sort+block", "rowsort+block", "2x cg2"]
    for fixture, extra in (("sdm-100-50.data", ["csr-f64", "csr-f64 At"]), ("sbm-100-50.data", [])):
        for flags in (["-r", "-b", "8"], ["-r", "-d"], ["-r", "-t", "-c"]):
            p = subprocess.run([exe, "-f", os.path.join(S.GOLDEN, fixture)] + flags, capture_output=True, text=True,
                               timeout=120)
            assert p.returncode == 0, p.stderr
            got = [ln.split("]")[0][1:] for ln in p.stdout.splitlines() if ln.startswith("[") and "Wall:" in ln]
            want = list(labels)
            if "-c" in flags:
                want.insert(want.index("4xblock"), "cg solver")
            assert got == want + extra, (fixture, flags, got)


@pytest.mark.parametrize("shape", [(1_000_000, 1_000_000, 8, True), (700_000, 2_000_000, 12, False), (300_000, 600_000, 40, True)])
def test_tiled_auto_geometry_midsize_vs_oracle(hip, shape):
    """matrices big enough for the format builder to choose the L2-tiled kernel by itself (x > 3 MB, > 4 M
    non-zeros): every row against the oracle, row-scaled 1e-12 bound; pattern-only + integer x bit-exact"""
    import torch
    from libfastsparse_amd import capi
    from oracle import pysynth
    nrow, ncol, per, valued = shape
    rp, cc, vv = capi.synth_uniform(nrow, ncol, per, 0xABC + nrow, valued=valued)
    A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv, borrow=True)
    hrp, hcc, hvv = pysynth.uniform(nrow, ncol, per, 0xABC + nrow, valued=valued)
    y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
    xs = S.x_sin(ncol)
    A.spmv(y, torch.from_numpy(xs).cuda(), capi.current_stream())
    ref = O.csr_mul(nrow, hrp, hcc, hvv, xs)
    scale = O.csr_abs_scale(nrow, hrp, hcc, hvv, xs)
    assert np.all(np.abs(y.cpu().numpy() - ref) <= TOL * np.maximum(scale, 1e-300))
    xi = S.x_int(9, ncol)
    A.spmv(y, torch.from_numpy(xi).cuda(), capi.current_stream())
    ref = O.csr_mul(nrow, hrp, hcc, hvv, xi)
    if valued:
        scale = O.csr_abs_scale(nrow, hrp, hcc, hvv, xi)
        assert np.all(np.abs(y.cpu().numpy() - ref) <= TOL * np.maximum(scale, 1e-300))
    else:
        assert np.array_equal(y.cpu().numpy(), ref)
    # two / three right-hand sides go through the tiled kernel column by column (strided X / Y)
    for k in (2, 3):
        X = S.X_sin(ncol, k)
        Y = torch.full((nrow, k), -1.0, dtype=torch.float64, device="cuda")
        A.spmm(Y, torch.from_numpy(X).cuda(), k, capi.current_stream())
        Yref = O.csr_mul_n(nrow, hrp, hcc, hvv, X, k)
        Yg = Y.cpu().numpy()
        for j in range(k):
            sc = O.csr_abs_scale(nrow, hrp, hcc, hvv, np.ascontiguousarray(X[:, j]))
            assert np.all(np.abs(Yg[:, j] - Yref[:, j]) <= TOL * np.maximum(sc, 1e-300)), (k, j)
    A.build_transpose(capi.current_stream())
    z = torch.full((ncol,), -1.0, dtype=torch.float64, device="cuda")
    xt = S.x_sin(nrow, 11.0, -0.2)
    A.spmv(z, torch.from_numpy(xt).cuda(), capi.current_stream(), transposed=True)
    rows = np.repeat(np.arange(nrow, dtype=np.int32), per)
    zref = O.coo_tmul(ncol, rows, hcc, hvv, xt)
    zscale = O.coo_tmul(ncol, rows, hcc, None if hvv is None else np.abs(hvv), np.abs(xt))
    assert np.all(np.abs(z.cpu().numpy() - zref) <= TOL * np.maximum(zscale, 1e-300))


def test_dropin_cache_invalidation(hip):
    """the side table keyed by the host struct: a matrix changed in place is re-uploaded (fingerprint or
    fs_invalidate), a freed one is dropped"""
    import ctypes as C
    be = hip.HipDropinBackend()
    c = BY_NAME["syn_dup_1024"]
    rows, cols = c.rows.copy(), c.cols.copy()
    A = hip.SBM(c.nrow, c.ncol, len(rows), rows.ctypes.data_as(hip.ip), cols.ctypes.data_as(hip.ip))
    x = S.x_int(4, c.ncol)
    y = np.full(c.nrow, -1.0)
    f = be.L.A_mul_B
    f.restype = None
    f(y.ctypes.data_as(hip.dp), C.byref(A), x.ctypes.data_as(hip.dp))
    assert np.array_equal(y, O.coo_mul(c.nrow, rows, cols, None, x))
    cols[:] = (cols + 1) % c.ncol                      # mutate in place: same pointers, new content
    be.L.fs_invalidate(C.byref(A))
    f(y.ctypes.data_as(hip.dp), C.byref(A), x.ctypes.data_as(hip.dp))
    assert np.array_equal(y, O.coo_mul(c.nrow, rows, cols, None, x))
    rows[:] = rows[::-1].copy()                        # no invalidate: the sampled fingerprint catches it
    cols[:] = cols[::-1].copy()
    f(y.ctypes.data_as(hip.dp), C.byref(A), x.ctypes.data_as(hip.dp))
    assert np.array_equal(y, O.coo_mul(c.nrow, rows, cols, None, x))
    be.L.fs_release_all()


def test_cbcsr_lds_staging_paths(hip):
    """cbcsr kernel with the x tile staged in LDS (forced), read from L2 (forced) and by the heuristic: same bits"""
    from libfastsparse_amd import capi
    be = hip.HipDeviceBackend()
    c = BY_NAME["syn_u16_2048"]
    x = c.xs["bench"]
    nb, rp, cc = O.coo_to_cbcsr(512, c.nrow, c.ncol, c.rows, c.cols)
    ref = O.cbcsr_mul(c.nrow, nb, rp, cc, x)
    for mode in (4, 5, 0):
        capi.set_option("spmv_kernel", mode)
        try:
            y = be.cbcsr_mul(c.nrow, c.ncol, c.rows, c.cols, 512, x)
        finally:
            capi.set_option("spmv_kernel", 0)
        assert np.array_equal(y, ref), mode       # cell sums added block by block: the one-thread CPU order


def test_csr_create_variants(hip):
    """fs_csr_create: host arrays, device copy, device borrow, and a borrow request on mis-aligned device
    arrays (falls back to a copy) all give the same product"""
    import torch
    from libfastsparse_amd import capi
    c = BY_NAME["syn_dup_1024"]
    rp, cc, vv = O.coo_to_csr(c.nrow, c.rows, c.cols, c.vals)
    x = c.xs["int"]
    ref = O.csr_mul(c.nrow, rp, cc, vv, x)
    xd = torch.from_numpy(x).cuda()
    drp, dcc, dvv = (torch.from_numpy(a).cuda() for a in (rp, cc, vv))
    pad_c = torch.empty(len(cc) + 1, dtype=torch.int32, device="cuda")
    pad_v = torch.empty(len(vv) + 1, dtype=torch.float64, device="cuda")
    pad_c[1:] = dcc
    pad_v[1:] = dvv
    variants = [capi.Matrix.from_csr(c.nrow, c.ncol, rp, cc, vv),                       # host arrays
                capi.Matrix.from_csr(c.nrow, c.ncol, drp, dcc, dvv),                    # device, copied
                capi.Matrix.from_csr(c.nrow, c.ncol, drp, dcc, dvv, borrow=True),       # device, in place
                capi.Matrix.from_csr(c.nrow, c.ncol, drp, pad_c[1:], pad_v[1:], borrow=True)]   # 4-byte aligned cols
    capi.set_option("strict_order", 1)
    try:
        for m in variants:
            y = torch.full((c.nrow,), -1.0, dtype=torch.float64, device="cuda")
            m.spmv(y, xd, capi.current_stream())
            assert np.array_equal(y.cpu().numpy(), ref)
    finally:
        capi.set_option("strict_order", 0)
    assert variants[0].algorithmic_bytes() == 12 * len(cc) + 4 * (c.nrow + 1) + 8 * c.nrow + 8 * c.ncol


def test_error_paths_return_codes(hip):
    """the device layer reports, it does not crash: NULL handles, k < 1, transpose not built"""
    import torch
    from libfastsparse_amd import capi
    L = capi.lib()
    c = BY_NAME["kat_sdm_6x4"]
    rp, cc, vv = O.coo_to_csr(c.nrow, c.rows, c.cols, c.vals)
    m = capi.Matrix.from_csr(c.nrow, c.ncol, rp, cc, vv)
    y = torch.zeros(c.ncol, dtype=torch.float64, device="cuda")
    x = torch.zeros(c.nrow, dtype=torch.float64, device="cuda")
    assert L.fs_spmv_t(m.h, y.data_ptr(), x.data_ptr(), None) == -4 and b"build_transpose" in L.fs_last_error()
    assert L.fs_spmv(None, y.data_ptr(), x.data_ptr(), None) == -2
    assert L.fs_spmm(m.h, y.data_ptr(), x.data_ptr(), 0, None) == -2
    assert L.fs_set_option(b"no_such_option", 1) == -2
    assert not L.fs_csr_create(-1, 1, 0, rp.ctypes.data, cc.ctypes.data, None, 0, 0)


def test_cbcsr_large_uses_cell_streaming(hip):
    """>= 1 M entries: cell sums by the streaming kernel + block-order combine; equals the one-thread-per-row
    kernels bit for bit with integer x, and the oracle's one-thread order under strict_order"""
    import torch
    from libfastsparse_amd import capi
    from oracle import pysynth
    nrow, ncol, per, cbs = 200_000, 300_000, 12, 65536
    rp, cc, _ = pysynth.uniform(nrow, ncol, per, 77, valued=False)
    rows = np.repeat(np.arange(nrow, dtype=np.int32), per)
    nb, crp, ccc = O.coo_to_cbcsr(cbs, nrow, ncol, rows, cc)
    m = capi.ColBlockMatrix(nrow, ncol, nb, cbs, torch.from_numpy(crp).cuda(), torch.from_numpy(ccc).cuda())
    y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
    xi = S.x_int(3, ncol)
    ref = O.cbcsr_mul(nrow, nb, crp, ccc, xi)
    for mode in (0, 5, 4):
        capi.set_option("spmv_kernel", mode)
        try:
            m.spmv(y, torch.from_numpy(xi).cuda(), capi.current_stream())
        finally:
            capi.set_option("spmv_kernel", 0)
        assert np.array_equal(y.cpu().numpy(), ref), mode
    xs = S.x_sin(ncol)
    ref = O.cbcsr_mul(nrow, nb, crp, ccc, xs)
    m.spmv(y, torch.from_numpy(xs).cuda(), capi.current_stream())
    assert np.max(np.abs(y.cpu().numpy() - ref)) <= TOL * per * 1.0
    capi.set_option("strict_order", 1)
    try:
        m.spmv(y, torch.from_numpy(xs).cuda(), capi.current_stream())
    finally:
        capi.set_option("strict_order", 0)
    assert np.array_equal(y.cpu().numpy(), ref)


def test_cbcsr_largest_runs_on_the_general_path(hip):
    """>= 4 M entries: the column-blocked matrix is also kept as a plain pattern-only CSR (rows in block-by-block
    order) and the product runs on the kernel the format builder chose; equals the cell-streaming path (mode 9) and the
    one-thread-per-row kernel bit for bit with integer x, the oracle within the fp64 bar, and under strict_order the
    oracle's one-thread order bit for bit (cell path)"""
    import torch
    from libfastsparse_amd import capi
    from oracle import pysynth
    nrow, ncol, per, cbs = 400_000, 250_000, 24, 65536
    rp, cc, _ = pysynth.uniform(nrow, ncol, per, 78, valued=False)
    rows = np.repeat(np.arange(nrow, dtype=np.int32), per)
    nb, crp, ccc = O.coo_to_cbcsr(cbs, nrow, ncol, rows, cc)
    m = capi.ColBlockMatrix(nrow, ncol, nb, cbs, torch.from_numpy(crp).cuda(), torch.from_numpy(ccc).cuda())
    y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
    xi = S.x_int(3, ncol)
    ref = O.cbcsr_mul(nrow, nb, crp, ccc, xi)
    for mode in (0, 9, 5):
        capi.set_option("spmv_kernel", mode)
        try:
            m.spmv(y, torch.from_numpy(xi).cuda(), capi.current_stream())
        finally:
            capi.set_option("spmv_kernel", 0)
        assert np.array_equal(y.cpu().numpy(), ref), mode
    xs = S.x_sin(ncol)
    ref = O.cbcsr_mul(nrow, nb, crp, ccc, xs)
    m.spmv(y, torch.from_numpy(xs).cuda(), capi.current_stream())
    assert np.max(np.abs(y.cpu().numpy() - ref)) <= TOL * per * 1.0
    capi.set_option("strict_order", 1)
    try:
        m.spmv(y, torch.from_numpy(xs).cuda(), capi.current_stream())
    finally:
        capi.set_option("strict_order", 0)
    assert np.array_equal(y.cpu().numpy(), ref)


def test_every_copy_on_extreme_distributions(hip):
    """matrices the format builder has to cut up -- one row holding almost everything, a heavy-tailed matrix with many
    empty rows, and a matrix whose entries sit in one column band, most of them in one column -- with the builder's own
    choice and with each copy forced (two-pass, LDS-staged, L2-tiled): every row against the oracle (row-scaled
    bound), integer x exact"""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(5)
    # (a) 1000 rows, row 7 has 5 M entries, the others 0-3
    ncol = 2_000_000
    lens = rng.integers(0, 4, 1000)
    lens[7] = 5_000_000
    rp = np.zeros(1001, np.int64)
    np.cumsum(lens, out=rp[1:])
    rp = rp.astype(np.int32)
    cc = rng.integers(0, ncol, int(rp[-1])).astype(np.int32)
    vv = rng.uniform(-1, 1, int(rp[-1]))
    # (b) 400 k rows, 30 % empty, Pareto lengths up to 200 k
    n2, ncol2 = 400_000, 3_000_000
    l2 = np.minimum((2.0 / rng.uniform(1e-6, 1, n2)).astype(np.int64), 200_000)
    l2[rng.uniform(size=n2) < 0.3] = 0
    rp2 = np.zeros(n2 + 1, np.int64)
    np.cumsum(l2, out=rp2[1:])
    rp2 = rp2.astype(np.int32)
    cc2 = rng.integers(0, ncol2, int(rp2[-1])).astype(np.int32)
    # (c) every entry in ONE column band and most of them in one column (a hot feature), 300 k rows
    n3, ncol3 = 300_000, 1_000_000
    l3 = rng.integers(8, 40, n3)
    rp3 = np.zeros(n3 + 1, np.int64)
    np.cumsum(l3, out=rp3[1:])
    rp3 = rp3.astype(np.int32)
    cc3 = (500_000 + rng.integers(0, 3000, int(rp3[-1]))).astype(np.int32)
    cc3[rng.uniform(size=cc3.size) < 0.6] = 501_234
    vv3 = rng.uniform(-1, 1, int(rp3[-1]))
    for forced in (None, "binning", "ldsx", "tiling"):
        for (nrow, nc, r_, c_, v_) in ((1000, ncol, rp, cc, vv), (n2, ncol2, rp2, cc2, None), (n3, ncol3, rp3, cc3, vv3)):
            if forced:
                capi.set_option(forced, 2)
            try:
                A = capi.Matrix.from_csr(nrow, nc, r_, c_, v_)
            finally:
                if forced:
                    capi.set_option(forced, 1)
            y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
            for x in (S.x_sin(nc), S.x_int(2, nc)):
                A.spmv(y, torch.from_numpy(x).cuda(), capi.current_stream())
                ref = O.csr_mul(nrow, r_, c_, v_, x)
                got = y.cpu().numpy()
                if v_ is None and np.all(x == np.round(x)):
                    assert np.array_equal(got, ref), (forced, A.kernel_name())
                else:
                    scale = O.csr_abs_scale(nrow, r_, c_, v_, x)
                    assert np.all(np.abs(got - ref) <= TOL * np.maximum(scale, 1e-300)), (forced, A.kernel_name())
            del A


@pytest.mark.parametrize("bin_rows", [0, 64, 1000])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_two_pass_kernels_vs_reference_golden(hip, case, bin_rows):
    """the two-pass (expand, then reduce) kernels, forced on: every entry point of every golden case, within the
    fp64 bar and bit-exact for pattern-only integer products; small panels so that the cases span many of them"""
    from libfastsparse_amd import capi
    capi.set_option("binning", 2)
    capi.set_option("bin_rows", bin_rows)
    capi.set_option("tile_split", 37 if bin_rows == 64 else 0)
    try:
        gold = np.load(os.path.join(S.GOLDEN, case.name + ".npz"))
        out = _cases.run_case(hip.HipDeviceBackend(), case, light=True)
        _check(out, gold, case.name, exact=False)
    finally:
        capi.set_option("binning", 1)
        capi.set_option("bin_rows", 0)
        capi.set_option("tile_split", 0)


@pytest.mark.parametrize("valued", [False, True])
def test_two_pass_kernels_many_bands_and_panels(hip, valued):
    """several column bands (the last one partial), hundreds of panels, ragged rows (0..60 entries, some cut into
    virtual rows), SpMV, the transposed product and two right-hand sides: every row against the oracle"""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(17)
    nrow, ncol = 50_000, 100_000          # 100000 = 6 x 16384 + 1696
    lens = rng.integers(0, 61, nrow)
    lens[rng.uniform(size=nrow) < 0.1] = 0
    lens[123] = 5000
    rp = np.zeros(nrow + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rp = rp.astype(np.int32)
    nnz = int(rp[-1])
    cc = rng.integers(0, ncol, nnz).astype(np.int32)
    cc[:50] = ncol - 1                      # the last column of the partial band
    vv = rng.uniform(-1, 1, nnz) if valued else None
    capi.set_option("binning", 2)
    capi.set_option("bin_rows", 500)
    capi.set_option("tile_split", 40)
    try:
        A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv)
        A.build_transpose(capi.current_stream())
        y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
        for x in (S.x_sin(ncol), S.x_int(4, ncol)):
            A.spmv(y, torch.from_numpy(x).cuda(), capi.current_stream())
            ref = O.csr_mul(nrow, rp, cc, vv, x)
            got = y.cpu().numpy()
            if not valued and np.all(x == np.round(x)):
                assert np.array_equal(got, ref)
            else:
                scale = O.csr_abs_scale(nrow, rp, cc, vv, x)
                assert np.all(np.abs(got - ref) <= TOL * np.maximum(scale, 1e-300))
        X = S.X_sin(ncol, 2)
        Y = torch.full((nrow, 2), -1.0, dtype=torch.float64, device="cuda")
        A.spmm(Y, torch.from_numpy(X).cuda(), 2, capi.current_stream())
        Yref = O.csr_mul_n(nrow, rp, cc, vv, X, 2)
        for j in range(2):
            sc = O.csr_abs_scale(nrow, rp, cc, vv, np.ascontiguousarray(X[:, j]))
            assert np.all(np.abs(Y.cpu().numpy()[:, j] - Yref[:, j]) <= TOL * np.maximum(sc, 1e-300)), j
        z = torch.full((ncol,), -1.0, dtype=torch.float64, device="cuda")
        xt = S.x_sin(nrow, 11.0, -0.2)
        A.spmv(z, torch.from_numpy(xt).cuda(), capi.current_stream(), transposed=True)
        rows = np.repeat(np.arange(nrow, dtype=np.int32), lens)
        zref = O.coo_tmul(ncol, rows, cc, vv, xt)
        zscale = O.coo_tmul(ncol, rows, cc, None if vv is None else np.abs(vv), np.abs(xt))
        assert np.all(np.abs(z.cpu().numpy() - zref) <= TOL * np.maximum(zscale, 1e-300))
    finally:
        capi.set_option("binning", 1)
        capi.set_option("bin_rows", 0)
        capi.set_option("tile_split", 0)


def test_two_pass_on_thousands_of_bands(hip):
    """x of 480 MB (3663 column bands, the last one partial), 40 M non-zeros: the format builder's own measured
    choice and the two-pass copy forced, both against the oracle on every row, integer x bit-exact"""
    import torch
    from libfastsparse_amd import capi
    from oracle import pysynth
    nrow, ncol, per = 1_000_000, 60_000_000, 40
    rp, cc, _ = capi.synth_uniform(nrow, ncol, per, 0x51, valued=False)
    hrp, hcc, _ = pysynth.uniform(nrow, ncol, per, 0x51, valued=False)
    xi, xs = S.x_int(9, ncol), S.x_sin(ncol)
    ref_i = O.csr_mul(nrow, hrp, hcc, None, xi)
    ref_s = O.csr_mul(nrow, hrp, hcc, None, xs)
    scale = O.csr_abs_scale(nrow, hrp, hcc, None, xs)
    y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
    chosen = []
    for binning in (1, 2):
        capi.set_option("binning", binning)
        try:
            A = capi.Matrix.from_csr(nrow, ncol, rp, cc, None, borrow=True)
        finally:
            capi.set_option("binning", 1)
        chosen.append(A.kernel_name())
        A.spmv(y, torch.from_numpy(xi).cuda(), capi.current_stream())
        assert np.array_equal(y.cpu().numpy(), ref_i), chosen
        A.spmv(y, torch.from_numpy(xs).cuda(), capi.current_stream())
        assert np.all(np.abs(y.cpu().numpy() - ref_s) <= TOL * np.maximum(scale, 1e-300)), chosen
        del A
    assert chosen[0] in ("two-pass", "tiled", "stream") and chosen[1] == "two-pass", chosen


def test_reproducible_option_and_tuning_switches(hip):
    """`reproducible`: the two-pass copy stays, its pass 2 then runs ONE wave per panel that adds in stream order
    (spmv_reduce_ordered_kernel), and repeated runs are bit-identical (the sixteen-wave pass 2 adds in arrival order: its
    bits may differ from run to run and from the ordered ones -- both within the rounding bar of the oracle); the option may be
    switched on after the matrix was created; the pass-1 unroll switches of the two-pass kernels change nothing but speed
    (pattern-only + integer x: exact)"""
    import torch
    from libfastsparse_amd import capi
    nrow, ncol, per = 600_000, 5_000_000, 16
    rp, cc, vv = capi.synth_uniform(nrow, ncol, per, 0x77, valued=True)
    x = torch.from_numpy(S.x_sin(ncol)).cuda()
    y1 = torch.empty(nrow, dtype=torch.float64, device="cuda")
    y2 = torch.empty_like(y1)
    capi.set_option("reproducible", 1)
    capi.set_option("binning", 2)
    try:
        A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv, borrow=True)
        assert A.kernel_name() == "two-pass"
        A.spmv(y1, x, capi.current_stream())
        for _ in range(5):
            y2.fill_(-1.0)
            A.spmv(y2, x, capi.current_stream())
            assert torch.equal(y1, y2)
        rpn, ccn, vvn = rp.cpu().numpy(), cc.cpu().numpy(), vv.cpu().numpy()
        ref = O.csr_mul(nrow, rpn, ccn, vvn, S.x_sin(ncol))
        sc = O.csr_abs_scale(nrow, rpn, ccn, vvn, S.x_sin(ncol))
        assert np.all(np.abs(y1.cpu().numpy() - ref) <= TOL * np.maximum(sc, 1e-300))
        # two and four right-hand sides: the k-column sweep stays too, its pass 2 ordered like the single-vector one
        for k in (2, 4):
            A.prepare(k, capi.current_stream())
            assert A.spmm_plan(k) == "k-column two-pass", A.spmm_plan(k)
            X = S.X_sin(ncol, k)
            Y1 = torch.full((nrow, k), -1.0, dtype=torch.float64, device="cuda")
            Y2 = torch.full((nrow, k), -2.0, dtype=torch.float64, device="cuda")
            A.spmm(Y1, torch.from_numpy(X).cuda(), k, capi.current_stream())
            for _ in range(3):
                A.spmm(Y2, torch.from_numpy(X).cuda(), k, capi.current_stream())
                assert torch.equal(Y1, Y2), k
            refk = O.csr_mul_n(nrow, rpn, ccn, vvn, X, k)
            for j in range(k):
                scj = O.csr_abs_scale(nrow, rpn, ccn, vvn, np.ascontiguousarray(X[:, j]))
                assert np.all(np.abs(Y1.cpu().numpy()[:, j] - refk[:, j]) <= TOL * np.maximum(scj, 1e-300)), (k, j)
        # the same handle without the option: the sixteen-wave pass 2, same sums to rounding
        capi.set_option("reproducible", 0)
        A.spmv(y2, x, capi.current_stream())
        assert np.all(np.abs(y2.cpu().numpy() - ref) <= TOL * np.maximum(sc, 1e-300))
        del A
    finally:
        capi.set_option("reproducible", 0)
        capi.set_option("binning", 1)
    capi.set_option("binning", 2)
    try:
        P = capi.Matrix.from_csr(nrow, ncol, rp, cc, None, borrow=True)
        assert P.kernel_name() == "two-pass"
        xi = torch.from_numpy(S.x_int(3, ncol)).cuda()
        P.spmv(y1, xi, capi.current_stream())
        for flags in (1, 2):
            capi.set_option("bin_flags", flags)
            P.spmv(y2, xi, capi.current_stream())
            assert torch.equal(y1, y2), flags
        # `reproducible` switched on later: the existing two-pass copy stays in use, with the ordered pass 2
        capi.set_option("bin_flags", 0)
        capi.set_option("reproducible", 1)
        assert P.kernel_name() == "two-pass"
        P.spmv(y2, xi, capi.current_stream())
        assert torch.equal(y1, y2)
        # and in parts (pass 2 by ranges of panels)
        if sum(b > a for a, b in zip(P.part_rows(3), P.part_rows(3)[1:])) >= 2:
            y2.fill_(-1.0)
            for part in range(3):
                P.spmv_part(y2, xi, part, 3, capi.current_stream())
            assert torch.equal(y1, y2)
    finally:
        capi.set_option("bin_flags", 0)
        capi.set_option("binning", 1)
        capi.set_option("reproducible", 0)


@pytest.mark.parametrize("geometry", [(64, 128, 0), (7, 33, 0), (300, 2048, 5), (0, 0, 0)])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_lds_staged_kernel_vs_reference_golden(hip, case, geometry):
    """the LDS-staged tiled kernel (x slice of every band in LDS), forced on, with small panels/bands so that every
    case spans many tiles and work items, and with rows cut into virtual rows: every entry point of every golden case"""
    from libfastsparse_amd import capi
    capi.set_option("ldsx", 2)
    capi.set_option("tile_rows", geometry[0])
    capi.set_option("tile_cols", geometry[1])
    capi.set_option("tile_split", geometry[2])
    try:
        gold = np.load(os.path.join(S.GOLDEN, case.name + ".npz"))
        out = _cases.run_case(hip.HipDeviceBackend(), case, light=True)
        _check(out, gold, case.name, exact=False)
    finally:
        capi.set_option("ldsx", 1)
        capi.set_option("tile_rows", 0)
        capi.set_option("tile_cols", 0)
        capi.set_option("tile_split", 0)


@pytest.mark.parametrize("valued", [False, True])
def test_lds_staged_kernel_dense_tiles(hip, valued):
    """a matrix with config 3's density (64 per row over 100 k columns: 49 bands of 2048, the last one partial),
    ragged rows, the kernel forced and chosen by the builder's own measurement: every row against the oracle; SpMV,
    two right-hand sides and the transposed product"""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(23)
    nrow, ncol = 400_000, 100_000
    lens = rng.integers(40, 90, nrow)
    lens[rng.uniform(size=nrow) < 0.05] = 0
    lens[777] = 30_000
    rp = np.zeros(nrow + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rp = rp.astype(np.int32)
    nnz = int(rp[-1])
    cc = rng.integers(0, ncol, nnz).astype(np.int32)
    cc[:64] = ncol - 1
    vv = rng.uniform(-1, 1, nnz) if valued else None
    xs_, xi_ = S.x_sin(ncol), S.x_int(4, ncol)
    ref_s, ref_i = O.csr_mul(nrow, rp, cc, vv, xs_), O.csr_mul(nrow, rp, cc, vv, xi_)
    sc_s, sc_i = O.csr_abs_scale(nrow, rp, cc, vv, xs_), O.csr_abs_scale(nrow, rp, cc, vv, xi_)
    chosen = []
    for forced in (2, 1):
        capi.set_option("ldsx", forced)
        try:
            A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv)
        finally:
            capi.set_option("ldsx", 1)
        chosen.append(A.kernel_name())
        y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
        # the two forms of the kernel on the same copy: slices by LDS DMA (default), through the registers (tiled_flags bit 2);
        # x 16-byte aligned (DMA) and 8 bytes off (falls back)
        xpad = torch.zeros(ncol + 1, dtype=torch.float64, device="cuda")
        xpad[1:] = torch.from_numpy(xs_).cuda()
        for flags, xdev in ((0, torch.from_numpy(xs_).cuda()), (4, torch.from_numpy(xs_).cuda()), (0, xpad[1:])):
            capi.set_option("tiled_flags", flags)
            try:
                y.fill_(-1.0)
                A.spmv(y, xdev, capi.current_stream())
            finally:
                capi.set_option("tiled_flags", 0)
            assert np.all(np.abs(y.cpu().numpy() - ref_s) <= TOL * np.maximum(sc_s, 1e-300)), (chosen, flags)
        A.spmv(y, torch.from_numpy(xs_).cuda(), capi.current_stream())
        assert np.all(np.abs(y.cpu().numpy() - ref_s) <= TOL * np.maximum(sc_s, 1e-300)), chosen
        A.spmv(y, torch.from_numpy(xi_).cuda(), capi.current_stream())
        if valued:
            assert np.all(np.abs(y.cpu().numpy() - ref_i) <= TOL * np.maximum(sc_i, 1e-300)), chosen
        else:
            assert np.array_equal(y.cpu().numpy(), ref_i), chosen
        if forced == 2:
            X = S.X_sin(ncol, 2)
            Y = torch.full((nrow, 2), -1.0, dtype=torch.float64, device="cuda")
            A.spmm(Y, torch.from_numpy(X).cuda(), 2, capi.current_stream())
            Yref = O.csr_mul_n(nrow, rp, cc, vv, X, 2)
            for j in range(2):
                sc = O.csr_abs_scale(nrow, rp, cc, vv, np.ascontiguousarray(X[:, j]))
                assert np.all(np.abs(Y.cpu().numpy()[:, j] - Yref[:, j]) <= TOL * np.maximum(sc, 1e-300)), j
        del A
    assert chosen[0] == "lds-staged", chosen


def test_fuzz_every_forced_copy_small_shapes(hip):
    """seeded fuzz over shapes (1 x 1 up to a few thousand x tens of thousands, empty rows, a long row, duplicates),
    forced copies and geometry overrides: A x, A' u and a two-column product of every kernel against the oracle"""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(int(os.environ.get("FS_FUZZ_SEED", "20261004")))
    opts = ("binning", "ldsx", "tiling", None)
    host_paths = set()
    try:
        for trial in range(int(os.environ.get("FS_FUZZ_TRIALS", "48"))):
            scale = int(os.environ.get("FS_FUZZ_SCALE", "1"))        # one-off runs at larger sizes
            nrow = int(rng.choice([1, 2, 17, 300, 1500, 5000])) * scale
            ncol = int(rng.choice([1, 3, 64, 900, 20000, 40000])) * scale
            maxlen = int(rng.choice([1, 4, 30, 200]))
            lens = rng.integers(0, maxlen + 1, nrow)
            if rng.uniform() < 0.5:
                lens[rng.uniform(size=nrow) < 0.3] = 0
            if rng.uniform() < 0.3:
                lens[int(rng.integers(0, nrow))] = int(rng.integers(1000, 6000))
            rp = np.zeros(nrow + 1, np.int64)
            np.cumsum(lens, out=rp[1:])
            rp = rp.astype(np.int32)
            nnz = int(rp[-1])
            cc = rng.integers(0, ncol, nnz).astype(np.int32)
            valued = bool(rng.uniform() < 0.5)
            vv = rng.uniform(-1, 1, nnz) if valued else None
            forced = opts[trial % 4]
            geo = {"tile_rows": int(rng.choice([0, 7, 64, 300])), "tile_cols": int(rng.choice([0, 33, 128, 2048])),
                   "bin_rows": int(rng.choice([0, 64, 1000])), "tile_split": int(rng.choice([0, 5, 37]))}
            for k_, v_ in geo.items():
                capi.set_option(k_, v_)
            if forced:
                capi.set_option(forced, 2)
            try:
                A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv)
                A.build_transpose(capi.current_stream())
            finally:
                if forced:
                    capi.set_option(forced, 1)
            what = (trial, nrow, ncol, nnz, valued, forced, geo, A.kernel_name(), A.kernel_name(True))
            x = S.x_sin(ncol) if valued else S.x_int(trial, ncol)
            y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
            A.spmv(y, torch.from_numpy(x).cuda(), capi.current_stream())
            ref = O.csr_mul(nrow, rp, cc, vv, x)
            if valued:
                sc_y = O.csr_abs_scale(nrow, rp, cc, vv, x)
                assert np.all(np.abs(y.cpu().numpy() - ref) <= TOL * np.maximum(sc_y, 1e-300)), what
            else:
                assert np.array_equal(y.cpu().numpy(), ref), what
            u = S.x_sin(nrow, 11.0, -0.2) if valued else S.x_int(trial + 1, nrow)
            z = torch.full((ncol,), -1.0, dtype=torch.float64, device="cuda")
            A.spmv(z, torch.from_numpy(u).cuda(), capi.current_stream(), transposed=True)
            rows = np.repeat(np.arange(nrow, dtype=np.int32), lens)
            zref = O.coo_tmul(ncol, rows, cc, vv, u)
            if valued:
                zs = O.coo_tmul(ncol, rows, cc, np.abs(vv), np.abs(u))
                assert np.all(np.abs(z.cpu().numpy() - zref) <= TOL * np.maximum(zs, 1e-300)), what
            else:
                assert np.array_equal(z.cpu().numpy(), zref), what
            X = S.X_sin(ncol, 2)
            Y = torch.full((nrow, 2), -1.0, dtype=torch.float64, device="cuda")
            A.spmm(Y, torch.from_numpy(X).cuda(), 2, capi.current_stream())
            Yref = O.csr_mul_n(nrow, rp, cc, vv, X, 2)
            for j in range(2):
                sc = O.csr_abs_scale(nrow, rp, cc, vv, np.ascontiguousarray(X[:, j]))
                assert np.all(np.abs(Y.cpu().numpy()[:, j] - Yref[:, j]) <= TOL * np.maximum(sc, 1e-300)), (what, j)
            # the same two products with HOST vectors (fs_spmv_host: ranges of bands / panels / workgroups where the copy allows)
            yh, zh = np.full(nrow, -1.0), np.full(ncol, -1.0)
            A.spmv_host(yh, x)
            host_paths.add(capi.lib().fs_debug_last_host_path())
            A.spmv_host(zh, u, transposed=True)
            host_paths.add(capi.lib().fs_debug_last_host_path())
            if valued:
                assert np.all(np.abs(yh - ref) <= TOL * np.maximum(sc_y, 1e-300)), what
                assert np.all(np.abs(zh - zref) <= TOL * np.maximum(zs, 1e-300)), what
            else:
                assert np.array_equal(yh, ref) and np.array_equal(zh, zref), what
            # fixed-order sums on whatever copy was kept: non-integer vectors, three runs bit-identical, every
            # element inside the row-scaled bar; a copy that cannot give them (an LDS-staged copy with a row too dense for one
            # wave) must have handed the product to another kernel -- the results decide, not the kernel's name
            xs_, us_ = S.x_sin(ncol), S.x_sin(nrow, 11.0, -0.2)
            rs_, rt_ = O.csr_mul(nrow, rp, cc, vv, xs_), O.coo_tmul(ncol, rows, cc, vv, us_)
            ss_ = np.maximum(O.csr_abs_scale(nrow, rp, cc, vv, xs_), 1e-300)
            st_ = np.maximum(O.coo_tmul(ncol, rows, cc, None if vv is None else np.abs(vv), np.abs(us_)), 1e-300)
            capi.set_option("reproducible", 1)
            try:
                runs = []
                for _ in range(3):
                    y.fill_(-1.0); z.fill_(-1.0)
                    A.spmv(y, torch.from_numpy(xs_).cuda(), capi.current_stream())
                    A.spmv(z, torch.from_numpy(us_).cuda(), capi.current_stream(), transposed=True)
                    runs.append((y.cpu().numpy().copy(), z.cpu().numpy().copy()))
                whatr = what + (A.kernel_name(), A.kernel_name(True))
                assert all(np.array_equal(runs[0][0], r_[0]) and np.array_equal(runs[0][1], r_[1]) for r_ in runs[1:]), whatr
                assert np.all(np.abs(runs[0][0] - rs_) <= TOL * ss_) and np.all(np.abs(runs[0][1] - rt_) <= TOL * st_), whatr
            finally:
                capi.set_option("reproducible", 0)
            del A
    finally:
        capi.set_option("reproducible", 0)
        for k_ in ("tile_rows", "tile_cols", "bin_rows", "tile_split"):
            capi.set_option(k_, 0)
    assert {0, 1, 2} <= host_paths or int(os.environ.get("FS_FUZZ_TRIALS", "48")) < 48, host_paths


@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_spmm_k_columns_in_one_two_pass_sweep(hip, k, valued):
    """k = 2, 3, 4 right-hand sides on the k-column two-pass copy (a k-column band of the row-major X in LDS, k products
    per entry: bcsr_A_mul_B2/_B4 csr.h:164-202, bsbm_A_mul_B2/_B4/_Bn sparse.h:276-336, csr_A_mul_Bn csr.h:441-465):
    4.8 M non-zeros, ragged rows (some cut into virtual rows), 3 M columns = hundreds of bands with a partial last one;
    every element against the oracle within the row-scaled bar, pattern-only + integer X bit for bit, and the copy
    really was the one that ran (the forced row kernel gives storage-order sums = the oracle's bits)"""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(100 + k)
    nrow, ncol = 400_000, 3_000_001
    lens = rng.integers(0, 25, nrow)
    lens[777] = 3000
    rp = np.zeros(nrow + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rp = rp.astype(np.int32)
    nnz = int(rp[-1])
    cc = rng.integers(0, ncol, nnz).astype(np.int32)
    cc[:40] = ncol - 1
    vv = rng.uniform(-1, 1, nnz) if valued else None
    st = capi.current_stream()
    capi.set_option("binning", 2)
    try:
        A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv)
        assert A.kernel_name() == "two-pass"
        # a product never builds: before fs_matrix_prepare the k columns run on what the handle holds (and are right) ...
        before = A.spmm_plan(k)
        assert before == ("two-pass per column" if k <= 3 else "row"), before
        X0 = S.X_sin(ncol, k)
        Y0 = torch.full((nrow, k), -1.0, dtype=torch.float64, device="cuda")
        A.spmm(Y0, torch.from_numpy(X0).cuda(), k, st)
        ref0 = O.csr_mul_n(nrow, rp, cc, vv, X0, k)
        for j in range(k):
            sc = O.csr_abs_scale(nrow, rp, cc, vv, np.ascontiguousarray(X0[:, j]))
            assert np.all(np.abs(Y0.cpu().numpy()[:, j] - ref0[:, j]) <= TOL * np.maximum(sc, 1e-300)), j
        held = A.device_bytes()
        assert held[2] == 0, held
        # ... prepare builds the k-column copy (idempotent), and from then on the one sweep serves this k
        A.prepare(k, st)
        A.prepare(k, st)
        assert A.spmm_plan(k) == "k-column two-pass", A.spmm_plan(k)
        held2 = A.device_bytes()
        per_entry = held2[2] / nnz
        kw = 4 if k == 4 else 2       # stored per padded entry: 2 + 2 bytes of local ids, 8 kw of products, 4 kw / 16 of gdst (+ 8 of values)
        assert held2[:2] == held[:2] and (4 + 8 * kw) <= per_entry <= 1.6 * (12.5 + 8 * kw), per_entry
        Xs = [X0]
        if not valued:
            Xs.append(np.ascontiguousarray(np.stack([S.x_int(31 + j, ncol) for j in range(k)], 1)))
        for X in Xs:
            Y = torch.full((nrow, k), -1.0, dtype=torch.float64, device="cuda")
            A.spmm(Y, torch.from_numpy(X).cuda(), k, st)
            got = Y.cpu().numpy()
            ref = O.csr_mul_n(nrow, rp, cc, vv, X, k)
            if not valued and np.all(X == np.round(X)):
                assert np.array_equal(got, ref)
            else:
                for j in range(k):
                    sc = O.csr_abs_scale(nrow, rp, cc, vv, np.ascontiguousarray(X[:, j]))
                    assert np.all(np.abs(got[:, j] - ref[:, j]) <= TOL * np.maximum(sc, 1e-300)), j
            capi.set_option("spmm_kernel", 1)        # row kernel: storage order, the oracle's bits
            try:
                A.spmm(Y, torch.from_numpy(X).cuda(), k, st)
            finally:
                capi.set_option("spmm_kernel", 0)
            assert np.array_equal(Y.cpu().numpy(), ref)
            if valued:
                assert not np.array_equal(got, ref), "the k-column sweep adds band-major: identical bits mean it did not run"
    finally:
        capi.set_option("binning", 1)


@pytest.mark.parametrize("k", [2, 4, 7, 16, 32, 40])
def test_spmm_matrix_core_experiment(hip, k):
    """spmm_kernel = 4: the v_mfma_f64_16x16x4_f64 row kernel (one wave per row, the row's values in row 0 of A, four
    gathered X rows as B).  Same results as the row kernel to rounding (the instruction fuses multiply and add), bit
    for bit for pattern-only matrices with integer X; empty rows, one long row, k not a multiple of 16"""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(7 * k)
    nrow, ncol = 30_000, 20_000
    lens = rng.integers(0, 40, nrow)
    lens[5] = 1234
    lens[rng.uniform(size=nrow) < 0.05] = 0
    rp = np.zeros(nrow + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rp = rp.astype(np.int32)
    nnz = int(rp[-1])
    cc = rng.integers(0, ncol, nnz).astype(np.int32)
    st = capi.current_stream()
    capi.set_option("spmm_kernel", 4)
    try:
        for vv, X in ((rng.uniform(-1, 1, nnz), S.X_sin(ncol, k)),
                      (None, np.ascontiguousarray(np.stack([S.x_int(3 + j, ncol) for j in range(k)], 1)))):
            A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv)
            Y = torch.full((nrow, k), -1.0, dtype=torch.float64, device="cuda")
            A.spmm(Y, torch.from_numpy(X).cuda(), k, st)
            got = Y.cpu().numpy()
            ref = O.csr_mul_n(nrow, rp, cc, vv, X, k)
            if vv is None:
                assert np.array_equal(got, ref)
            else:
                for j in range(k):
                    sc = O.csr_abs_scale(nrow, rp, cc, vv, np.ascontiguousarray(X[:, j]))
                    assert np.all(np.abs(got[:, j] - ref[:, j]) <= TOL * np.maximum(sc, 1e-300)), j
    finally:
        capi.set_option("spmm_kernel", 0)


@pytest.mark.parametrize("shape", [(300_000, 300_000, 16, True), (400_000, 60_000, 64, False), (30_000, 30_000, 8, True)])
def test_products_can_be_captured_in_a_hip_graph_and_replayed(hip, shape):
    """fs_spmv / fs_spmv_t only launch (no allocation, no wait, no host-side state that a replay would miss), so a caller may
    capture them on its stream into a HIP graph and replay it: y = A x, z = A' y captured once, replayed on fresh outputs,
    against the eager products (same kernels, same order: bit-identical for the pattern-only case, to rounding of the atomic
    order otherwise).  (tools/graph_probe.py times eager against replay: no gain on this runtime, 31 vs 35 us for a pair of
    small products -- so the library itself does not use graphs.)"""
    import torch
    from libfastsparse_amd import capi
    n, m, per, valued = shape
    rp, cc, vv = capi.synth_uniform(n, m, per, 21, valued=valued)
    A = capi.Matrix.from_csr(n, m, rp, cc, vv, borrow=True)
    A.build_transpose(capi.current_stream())
    x = ((torch.arange(m, device="cuda") % 13) - 6).to(torch.float64) if not valued else torch.sin(torch.arange(m, device="cuda", dtype=torch.float64))
    y, z = torch.empty(n, device="cuda", dtype=torch.float64), torch.empty(m, device="cuda", dtype=torch.float64)
    yref, zref = torch.empty_like(y), torch.empty_like(z)
    A.spmv(yref, x, capi.current_stream())
    A.spmv(zref, yref, capi.current_stream(), transposed=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        A.spmv(y, x, capi.current_stream())
        A.spmv(z, y, capi.current_stream(), transposed=True)
        s.synchronize()
        with torch.cuda.graph(g, stream=s):
            A.spmv(y, x, capi.current_stream())
            A.spmv(z, y, capi.current_stream(), transposed=True)
    for _ in range(2):
        y.fill_(-1.0)
        z.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        if valued:
            assert torch.allclose(y, yref, rtol=0, atol=1e-11 * per) and torch.allclose(z, zref, rtol=1e-12, atol=1e-9)
        else:
            assert torch.equal(y, yref) and torch.equal(z, zref)


def test_lds_staged_panels_are_cut_to_equal_heights(hip):
    """Few rows, many columns (the shape of config 3 transposed): the LDS-staged copy takes full-height panels and cuts them
    into chunks.  Every panel sweeps every band whatever it holds, so a remainder panel of a few hundred rows costs as many
    phases as a full one (round 3: 1 M rows under a limit of 14 272 left one of 960 rows and the product took 1.10 ms instead
    of 0.75): panels must be as equal as the row count allows.  2 x 14 336 + 300 rows -> three panels of 9 658 / 9 658 / 9 656
    rows, not 14 336 / 14 336 / 300.  Product against the oracle, bit for bit on integer x."""
    import ctypes as C
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(99)
    nrow, ncol, per = 2 * 14336 + 300, 300_000, 200
    rp = (np.arange(nrow + 1, dtype=np.int64) * per).astype(np.int32)
    cc = rng.integers(0, ncol, nrow * per).astype(np.int32)
    for k, v in (("ldsx", 2), ("tiling", 0), ("binning", 0)):
        capi.set_option(k, v)
    try:
        A = capi.Matrix.from_csr(nrow, ncol, rp, cc, None)
    finally:
        for k, v in (("ldsx", 1), ("tiling", 1), ("binning", 1)):
            capi.set_option(k, v)
    assert A.kernel_name() == "lds-staged"
    L = capi.lib()
    L.fs_debug_tiled_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    g = (C.c_int * 6)()
    assert L.fs_debug_tiled_geometry(A.h, g) == 0
    R, P = int(g[0]), int(g[2])
    assert P == 3 and R == -(-nrow // 3), (R, P)
    x = S.x_int(12, ncol)
    y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
    A.spmv(y, torch.from_numpy(x).cuda(), capi.current_stream())
    assert np.array_equal(y.cpu().numpy(), O.csr_mul(nrow, rp, cc, None, x))


@pytest.mark.parametrize("k", [2, 4, 6, 8, 12, 16, 32, 40, 130])
def test_spmm_row_kernel_with_16_byte_loads_has_the_bits_of_the_row_loop(hip, k):
    """spmm_wide_kernel (two columns per lane, dwordx4 loads, up to sixteen X rows in flight; the default for even k from 4 to
    14 with 16-byte aligned X and Y, forced here by spmm_wide = 1): every column adds in storage order, so VALUED products with
    real X must equal the oracle's row loop (csr.h:441-465) bit for bit; rows of 0 .. 39 entries, one of 1234 (several steps of
    the entry loop), k / 2 not a power of two, k > 128 (more than one pass over the columns); and an X that is only 8-byte
    aligned must fall back to the one-column kernel with the same bits"""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(11 * k)
    nrow, ncol = 30_000, 20_000
    lens = rng.integers(0, 40, nrow)
    lens[5] = 1234
    lens[rng.uniform(size=nrow) < 0.05] = 0
    rp = np.zeros(nrow + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rp = rp.astype(np.int32)
    nnz = int(rp[-1])
    cc = rng.integers(0, ncol, nnz).astype(np.int32)
    st = capi.current_stream()
    capi.set_option("spmm_kernel", 1)
    capi.set_option("spmm_wide", 1)
    try:
        for vv in (rng.uniform(-1, 1, nnz), None):
            X = S.X_sin(ncol, k)
            A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv)
            ref = O.csr_mul_n(nrow, rp, cc, vv, X, k)
            Y = torch.full((nrow, k), -1.0, dtype=torch.float64, device="cuda")
            A.spmm(Y, torch.from_numpy(X).cuda(), k, st)
            assert np.array_equal(Y.cpu().numpy(), ref)
            buf = torch.zeros(ncol * k + 1, dtype=torch.float64, device="cuda")      # X at an odd multiple of 8 bytes
            buf[1:] = torch.from_numpy(X).cuda().reshape(-1)
            Y.fill_(-1.0)
            A.spmm(Y, buf[1:], k, st)
            assert np.array_equal(Y.cpu().numpy(), ref)
    finally:
        capi.set_option("spmm_kernel", 0)
        capi.set_option("spmm_wide", 0)


def _csr_struct(hip, nrow, ncol, rp, cc, vv):
    return hip.CSR(nrow, ncol, len(cc), hip._ip(rp), hip._ip(cc), hip._dp(vv))


def test_dropin_cache_sees_one_edited_entry(hip):
    """an entry edited in place at the same pointers.  Matrices up to 8 MB are hashed in full on every call,
    so ONE changed value or column is seen without fs_invalidate; beyond that the fingerprint is sampled and such an edit
    needs fs_invalidate (asserted here, so the documented behaviour is pinned) or FS_STRICT_CACHE=1 (next test)"""
    import ctypes as C
    L = hip.HipDropinBackend().L
    L.csr_A_mul_B.restype = None
    rng = np.random.default_rng(5)
    for nrow, per, expect_fresh in ((20_000, 10, True), (150_000, 10, False)):       # 2.4 MB / 18 MB of arrays
        ncol = nrow
        rp = (np.arange(nrow + 1, dtype=np.int64) * per).astype(np.int32)
        cc = rng.integers(0, ncol, nrow * per).astype(np.int32)
        vv = rng.uniform(-1, 1, nrow * per)
        A = _csr_struct(hip, nrow, ncol, rp, cc, vv)
        x = S.x_int(4, ncol)
        y = np.full(nrow, -1.0)
        L.csr_A_mul_B(hip._dp(y), C.byref(A), hip._dp(x))
        ref0 = O.csr_mul(nrow, rp, cc, vv, x)
        assert np.all(np.abs(y - ref0) <= TOL * O.csr_abs_scale(nrow, rp, cc, vv, x))
        k = 777 * per + 3                                   # not one of the 2048 strided samples, not an end
        assert k % max(1, (nrow * per) // 2048) != 0
        vv[k] += 1000.0
        cc[k] = (cc[k] + 1) % ncol
        ref1 = O.csr_mul(nrow, rp, cc, vv, x)
        assert ref1[777] != ref0[777]
        L.csr_A_mul_B(hip._dp(y), C.byref(A), hip._dp(x))
        if expect_fresh:
            assert abs(y[777] - ref1[777]) <= 1e-9, "a small matrix is hashed in full: the edit must be seen"
        else:
            assert abs(y[777] - ref0[777]) <= 1e-9, "sampled fingerprint: the stale copy is what runs (documented)"
            L.fs_invalidate(C.byref(A))
            L.csr_A_mul_B(hip._dp(y), C.byref(A), hip._dp(x))
            assert abs(y[777] - ref1[777]) <= 1e-9
        L.fs_invalidate(C.byref(A))


@pytest.mark.parametrize("nnz", [3, 7, 45, 8 * 1000 + 5])
def test_dropin_cache_sees_edits_in_short_and_ragged_arrays(hip, nnz):
    """the full fingerprint must cover EVERY byte.  Arrays shorter than 32 bytes (3 ints, 3 doubles) are all
    "tail" for a 32-byte-block hash, and 8k + 5 entries leave 20 / 40 trailing bytes: an edit of the FIRST value or the
    FIRST column at unchanged pointers must be seen (it used to survive: only the last 8 bytes of the tail were hashed)"""
    import ctypes as C
    L = hip.HipDropinBackend().L
    L.csr_A_mul_B.restype = None
    rng = np.random.default_rng(nnz)
    nrow, ncol = 4, 11
    rp = np.array([0, nnz // 3, nnz // 3, nnz - 1, nnz], np.int32)
    cc = rng.integers(0, ncol - 1, nnz).astype(np.int32)
    vv = rng.integers(-5, 6, nnz).astype(np.float64)          # integers: every order of additions gives the same bits
    A = _csr_struct(hip, nrow, ncol, rp, cc, vv)
    x = np.arange(ncol, dtype=np.float64) + 1.0
    y = np.full(nrow, -1.0)
    L.csr_A_mul_B(hip._dp(y), C.byref(A), hip._dp(x))
    assert np.array_equal(y, O.csr_mul(nrow, rp, cc, vv, x))
    for edit in ("vals", "cols", "vals_tail", "cols_tail"):
        i = 0 if not edit.endswith("tail") else max(nnz - 3, 0)        # inside the trailing bytes, not the last word
        if edit.startswith("vals"):
            vv[i] += 3.0
        else:
            cc[i] = cc[i] + 1
        L.csr_A_mul_B(hip._dp(y), C.byref(A), hip._dp(x))
        assert np.array_equal(y, O.csr_mul(nrow, rp, cc, vv, x)), (nnz, edit)
    L.fs_invalidate(C.byref(A))


def test_dropin_blocked_matrix_without_rows(hip):
    """new_bsbm of a matrix with nrow == 0 has no blocks; bsbm_A_mul_B on it does nothing in the reference
    (sparse.h:259-273: the block loop runs zero times) and used to divide by zero in the side table's fingerprint"""
    import ctypes as C
    be = hip.HipDropinBackend()
    L = be.L
    s = be.sbm(0, 7, np.zeros(0, np.int32), np.zeros(0, np.int32))
    B = L.new_bsbm(C.byref(s), 8)
    assert B.contents.nblocks == 0
    y = np.full(1, -1.0)
    for f in (L.bsbm_A_mul_B, L.bsbm_A_mul_B2):
        f.restype = None
        f(hip._dp(y), B, hip._dp(np.ones(14)))
    assert y[0] == -1.0                      # nothing to write: y has no elements
    L.fs_invalidate(B)


@pytest.mark.parametrize("kind", ["two-pass", "two-pass cut rows", "lds-staged", "tiled", "stream"])
def test_product_in_parts_finishes_rows_range_by_range(hip, kind):
    """fs_spmv_part / fs_spmv_part_rows (the all-gather overlapped inside one product needs the product
    to finish its rows range by range): for every kernel the row cuts are monotone from 0 to nrow, after parts 0 .. p the rows
    below rows[p + 1] are final (the others still hold the poison), and all parts together are fs_spmv bit for bit
    (pattern-only, integer x).  A kernel that cannot be cut does everything with part 0."""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(len(kind))
    opt, nrow, ncol, per = {"two-pass": ("binning", 4_000_000, 700_001, 3), "two-pass cut rows": ("binning", 3_600_000, 700_001, 3),
                            # panel kernels are cut between generations of resident workgroups: more panels than CUs
                            "lds-staged": ("ldsx", 4_000_000, 4_096, 6), "tiled": ("tiling", 4_000_000, 300_000, 5),
                            "stream": (None, 50_000, 20_000, 10)}[kind]
    lens = rng.integers(0, 2 * per, nrow)
    if kind == "two-pass cut rows":
        lens[[5, nrow // 2, nrow - 3]] = [70_000, 3_000, 900]        # cut into virtual rows; one spans several panels
    rp = np.zeros(nrow + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rp = rp.astype(np.int32)
    cc = rng.integers(0, ncol, int(rp[-1])).astype(np.int32)
    st = capi.current_stream()
    if opt:
        capi.set_option(opt, 2)
    try:
        A = capi.Matrix.from_csr(nrow, ncol, rp, cc, None)
        assert A.kernel_name() == kind.split(" cut")[0], A.kernel_name()
        x = S.x_int(9, ncol)
        xd = torch.from_numpy(x).cuda()
        ref = O.csr_mul(nrow, rp, cc, None, x)
        for nparts in (1, 2, 4, 7):
            rows = A.part_rows(nparts)
            assert rows[0] == 0 and rows[-1] == nrow and all(a <= b for a, b in zip(rows, rows[1:])), rows
            if kind != "stream" and nparts > 1:
                assert sum(b > a for a, b in zip(rows, rows[1:])) >= 2, (kind, rows)     # it really is cut
            y = torch.full((nrow,), -7.0, dtype=torch.float64, device="cuda")
            for p in range(nparts):
                A.spmv_part(y, xd, p, nparts, st)
                got = y.cpu().numpy()
                assert np.array_equal(got[:rows[p + 1]], ref[:rows[p + 1]]), (kind, nparts, p)
            assert np.array_equal(y.cpu().numpy(), ref)
    finally:
        if opt:
            capi.set_option(opt, 1)


@pytest.mark.parametrize("geometry", [1, 2])
@pytest.mark.parametrize("valued", [False, True])
def test_longest_rows_outside_the_two_pass_copy(hip, valued, geometry):
    """LongRows (round 3; BASELINE config 5's heavy tail): the longest rows of a power-law matrix are taken out of the two-pass
    copy and summed in ONE pass with their accumulators in LDS next to the band of x.  Forced here on a small matrix (rows from
    64 entries on, more candidates than the 3072 accumulators: the longest are taken), every row against the oracle; the
    product in parts; a strided 3-column product (one sweep per column); and the same matrix without the long-row path."""
    import ctypes as C
    import torch
    from libfastsparse_amd import capi
    from oracle import pysynth
    nrow, ncol = 300_000, 400_003
    rp, cc, vv = pysynth.powerlaw(nrow, ncol, 2.3, 150_000, 0x10C6, valued=valued)
    if not valued:
        vv = None
    st = capi.current_stream()
    L = capi.lib()
    x = S.x_int(3, ncol) if not valued else np.sin(7.0 * np.arange(ncol) + 0.3)
    ref = O.csr_mul(nrow, rp, cc, vv, x)
    scale = O.csr_abs_scale(nrow, rp, cc, vv, x) if valued else None

    def check(got, what):
        if valued:
            assert np.all(np.abs(got - ref) <= TOL * np.maximum(scale, 1e-300)), what
        else:
            assert np.array_equal(got, ref), what

    capi.set_option("binning", 2)
    try:
        for mode in (2, 0):
            capi.set_option("long_rows", mode)
            capi.set_option("long_min_len", 64)
            capi.set_option("long_geometry", geometry)          # 1: 16384-column band + 3072 rows, 2: 8192 + 12032 rows
            A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv)
            assert A.kernel_name() == "two-pass"
            info = (C.c_int64 * 2)()
            L.fs_debug_long_rows.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
            assert L.fs_debug_long_rows(A.h, 0, info) == 0
            lens = np.diff(rp)
            if mode == 2:
                cand = int((lens >= 64).sum())
                cap = 3072 if geometry == 1 else 12032
                want = min(cand, cap)
                assert geometry == 2 or cand > cap                                   # geometry 1 exercises the cap: the longest 3072 rows
                assert info[0] == want, (info[0], want)
                assert info[1] >= int(np.sort(lens)[-want:].sum())                   # all their entries (+ padding)
            else:
                assert info[0] == 0
            xd = torch.from_numpy(x).cuda()
            y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
            A.spmv(y, xd, st)
            check(y.cpu().numpy(), ("whole", mode))
            rows = A.part_rows(3)
            yp = torch.full((nrow,), -7.0, dtype=torch.float64, device="cuda")
            for part in range(3):
                A.spmv_part(yp, xd, part, 3, st)
                got = yp.cpu().numpy()
                if valued:
                    assert np.all(np.abs(got[:rows[part + 1]] - ref[:rows[part + 1]]) <= TOL * np.maximum(scale[:rows[part + 1]], 1e-300))
                else:
                    assert np.array_equal(got[:rows[part + 1]], ref[:rows[part + 1]]), (mode, part)
            X = np.ascontiguousarray(np.stack([x, 2.0 * x, -x], 1))
            Y = torch.full((nrow, 3), -1.0, dtype=torch.float64, device="cuda")
            assert A.spmm_plan(3) == "two-pass per column"
            A.spmm(Y, torch.from_numpy(X).cuda(), 3, st)
            Yh = Y.cpu().numpy()
            for j, f in enumerate((1.0, 2.0, -1.0)):
                if valued:
                    assert np.all(np.abs(Yh[:, j] - f * ref) <= 2 * TOL * np.maximum(scale, 1e-300)), j
                else:
                    assert np.array_equal(Yh[:, j], f * ref), j
            yh = np.full(nrow, -1.0)
            A.spmv_host(yh, x)                                   # host vectors: copy, product, copy (no band ranges with long rows)
            check(yh, ("host", mode))
            if mode == 2:
                # fixed-order sums: the long rows STAY on their path -- every long row belongs to one wave of a
                # workgroup, the workgroups' sums are added in workgroup order -- and repeated products are bit-identical
                xs_ = np.sin(7.0 * np.arange(ncol) + 0.3)
                ref_s, sc_s = O.csr_mul(nrow, rp, cc, vv, xs_), O.csr_abs_scale(nrow, rp, cc, vv, xs_)
                xsd = torch.from_numpy(xs_).cuda()
                capi.set_option("reproducible", 1)
                try:
                    assert A.kernel_name() == "two-pass"
                    assert L.fs_debug_long_rows(A.h, 0, info) == 0 and info[0] == want
                    runs = []
                    for _ in range(4):
                        y.fill_(-1.0)
                        A.spmv(y, xsd, st)
                        runs.append(y.cpu().numpy().copy())
                    assert all(np.array_equal(runs[0], r_) for r_ in runs[1:]), "fixed-order long rows differ between runs"
                    assert np.all(np.abs(runs[0] - ref_s) <= TOL * np.maximum(sc_s, 1e-300))
                    A2 = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv)          # a second build: the same order of additions
                    y.fill_(-1.0)
                    A2.spmv(y, xsd, st)
                    assert np.array_equal(y.cpu().numpy(), runs[0]), "a second build of the long-row copy adds in another order"
                    del A2
                finally:
                    capi.set_option("reproducible", 0)
                y.fill_(-1.0)
                A.spmv(y, xsd, st)                               # arrival order: the same sums to rounding
                assert np.all(np.abs(y.cpu().numpy() - ref_s) <= TOL * np.maximum(sc_s, 1e-300))
            del A
    finally:
        for k_, v_ in (("binning", 1), ("long_rows", 1), ("long_min_len", 0), ("long_geometry", 0)):
            capi.set_option(k_, v_)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_k_column_product_in_parts(hip, k):
    """fs_spmm_part / fs_spmm_part_rows: the one-sweep kernel of k = 2, 4 finishes its rows by generations of pass-2 panels
    (the block-CG iteration's exchange rides on that); k = 3 (two sweeps) and unprepared handles do everything with part 0.
    Pattern-only, integer X: every part's rows and the whole against the oracle, bit for bit."""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(50 + k)
    nrow, ncol, per = 3_000_000, 500_001, 3
    rp = (np.arange(nrow + 1, dtype=np.int64) * per).astype(np.int32)
    cc = rng.integers(0, ncol, nrow * per).astype(np.int32)
    st = capi.current_stream()
    capi.set_option("binning", 2)
    try:
        A = capi.Matrix.from_csr(nrow, ncol, rp, cc, None)
        X = np.ascontiguousarray(np.stack([S.x_int(7 + j, ncol) for j in range(k)], 1))
        ref = O.csr_mul_n(nrow, rp, cc, None, X, k)
        Xd = torch.from_numpy(X).cuda()
        for prepared in (False, True):
            if prepared:
                A.prepare(k, st)
            rows = A.part_rows(3, k=k)
            assert rows[0] == 0 and rows[-1] == nrow and all(a <= b for a, b in zip(rows, rows[1:])), rows
            cutk = prepared and k in (2, 4)
            assert (sum(b > a for a, b in zip(rows, rows[1:])) >= 2) == cutk, (k, prepared, rows)
            Y = torch.full((nrow, k), -7.0, dtype=torch.float64, device="cuda")
            for part in range(3):
                A.spmm_part(Y, Xd, k, part, 3, st)
                assert np.array_equal(Y.cpu().numpy()[:rows[part + 1]], ref[:rows[part + 1]]), (k, prepared, part)
            assert np.array_equal(Y.cpu().numpy(), ref)
    finally:
        capi.set_option("binning", 1)


def test_copy_segments_unpacks_a_padded_gather(hip):
    """fs_copy_segments: the one-launch unpack of the padded receive buffer of an all-gather of unequal shards"""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(3)
    counts = [0, 1, 1000, 123_457, 5, 0, 70_001]
    src_off = np.cumsum([0] + [c + 17 for c in counts[:-1]])
    dst_off = np.cumsum([3] + [c + 2 for c in counts[:-1]])
    src = rng.uniform(size=int(src_off[-1] + counts[-1] + 17))
    dst = np.full(int(dst_off[-1] + counts[-1] + 9), -1.0)
    want = dst.copy()
    for d, s_, c in zip(dst_off, src_off, counts):
        want[d:d + c] = src[s_:s_ + c]
    tab = torch.tensor(list(dst_off) + list(src_off) + counts, dtype=torch.int64, device="cuda")
    sd, dd = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    capi.check(capi.lib().fs_copy_segments(len(counts), tab.data_ptr(), max(counts), sd.data_ptr(), dd.data_ptr(),
                                           capi.current_stream()), "fs_copy_segments")
    assert np.array_equal(dd.cpu().numpy(), want)


@pytest.mark.parametrize("k", [2, 5])
def test_spmm_never_waits_prepare_decides(hip, k):
    """a matrix on the LDS-staged copy.  fs_spmm before fs_matrix_prepare runs one sweep per column (no
    timing of candidates inside the product any more); fs_matrix_prepare measures sweeps against the row kernel once and
    pins the plan; both give the oracle's result (row-scaled bar; pattern-only + integer X bit for bit)"""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(k)
    nrow, ncol, per = 60_000, 4_096, 40
    rp = (np.arange(nrow + 1, dtype=np.int64) * per).astype(np.int32)
    cc = rng.integers(0, ncol, nrow * per).astype(np.int32)
    st = capi.current_stream()
    capi.set_option("ldsx", 2)
    try:
        A = capi.Matrix.from_csr(nrow, ncol, rp, cc, None)
        assert A.kernel_name() == "lds-staged"
        X = np.ascontiguousarray(np.stack([S.x_int(11 + j, ncol) for j in range(k)], 1))
        ref = O.csr_mul_n(nrow, rp, cc, None, X, k)
        Y = torch.full((nrow, k), -1.0, dtype=torch.float64, device="cuda")
        # before prepare: nothing is allocated inside a product -- strided sweeps of the LDS-staged kernel (k = 2) or
        # the row kernel run on what the handle holds; prepare allocates the column-major scratch and measures
        assert A.spmm_plan(k) == ("lds-staged strided" if k == 2 else "row"), A.spmm_plan(k)
        assert A.device_bytes()[2] == 0
        A.spmm(Y, torch.from_numpy(X).cuda(), k, st)
        assert np.array_equal(Y.cpu().numpy(), ref)
        A.prepare(k, st)
        plan = A.spmm_plan(k)
        assert plan in ("lds-staged per column", "row") and (k != 2 or plan == "lds-staged per column"), plan
        Y.fill_(-1.0)
        A.spmm(Y, torch.from_numpy(X).cuda(), k, st)
        assert np.array_equal(Y.cpu().numpy(), ref)
        assert A.device_bytes()[2] >= 8 * k * (nrow + ncol)          # the column-major scratch is accounted for
    finally:
        capi.set_option("ldsx", 1)


def test_host_vector_product_waits_for_device_vector_products(hip):
    """fs_spmv returns right after an asynchronous launch on the caller's stream; fs_spmv_host runs on the
    handle's own non-blocking stream and shares the handle's scratch (the two-pass product stream).  It has to order itself
    behind the earlier launches: a burst of device-vector products on a side stream, then the host-vector product"""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(77)
    nrow, ncol, per = 300_000, 2_000_003, 16
    rp = (np.arange(nrow + 1, dtype=np.int64) * per).astype(np.int32)
    cc = rng.integers(0, ncol, nrow * per).astype(np.int32)
    capi.set_option("binning", 2)
    try:
        A = capi.Matrix.from_csr(nrow, ncol, rp, cc, None)
        assert A.kernel_name() == "two-pass"
        side = torch.cuda.Stream()
        x1, x2 = S.x_int(1, ncol), S.x_int(2, ncol)
        xd = torch.from_numpy(x1).cuda()
        yd = torch.empty(nrow, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for _ in range(30):
            A.spmv(yd, xd, side.cuda_stream)
        yh = np.full(nrow, -1.0)
        A.spmv_host(yh, x2)                                  # must not overlap the 30 products still in flight
        assert np.array_equal(yh, O.csr_mul(nrow, rp, cc, None, x2))
        side.synchronize()
        assert np.array_equal(yd.cpu().numpy(), O.csr_mul(nrow, rp, cc, None, x1))
    finally:
        capi.set_option("binning", 1)


def test_dropin_strict_cache_and_bounded_table_in_a_fresh_process(hip):
    """FS_STRICT_CACHE=1 (every array hashed in full on every call): the large-matrix edit of the previous test is
    seen without fs_invalidate.  FS_DROPIN_MAX_ENTRIES=3: the side table never holds more than 3 idle copies.
    free_sbm drops both copies (A_mul_B and At_mul_B handles) of a SparseBinaryMatrix."""
    import subprocess
    import sys
    code = r'''
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import _hipbackend as H
from oracle import pyoracle as O
L = H.HipDropinBackend().L
L.csr_A_mul_B.restype = None
rng = np.random.default_rng(5)
nrow = ncol = 150_000; per = 10
rp = (np.arange(nrow + 1, dtype=np.int64) * per).astype(np.int32)
cc = rng.integers(0, ncol, nrow * per).astype(np.int32)
vv = rng.uniform(-1, 1, nrow * per)
A = H.CSR(nrow, ncol, len(cc), H._ip(rp), H._ip(cc), H._dp(vv))
x = np.arange(ncol, dtype=np.float64) %% 7 - 3
y = np.full(nrow, -1.0)
L.csr_A_mul_B(H._dp(y), C.byref(A), H._dp(x))
k = 777 * per + 3
vv[k] += 1000.0
L.csr_A_mul_B(H._dp(y), C.byref(A), H._dp(x))
ref = O.csr_mul(nrow, rp, cc, vv, x)
assert abs(y[777] - ref[777]) <= 1e-9, (y[777], ref[777])
keep = []
for i in range(6):
    r2 = rp[: 1001].copy(); c2 = cc[: r2[-1]].copy(); v2 = vv[: r2[-1]].copy()
    B = H.CSR(1000, ncol, len(c2), H._ip(r2), H._ip(c2), H._dp(v2)); keep.append((B, r2, c2, v2))
    yy = np.empty(1000)
    L.csr_A_mul_B(H._dp(yy), C.byref(B), H._dp(x))
    assert np.allclose(yy, ref[:1000] if i < 0 else O.csr_mul(1000, r2, c2, v2, x))
assert L.fs_cache_entries() == 3, L.fs_cache_entries()
L.fs_release_all()
# free_sbm: both handles of a SparseBinaryMatrix go (arrays must be malloc'ed: free_sbm frees them)
libc = C.CDLL(None); libc.malloc.restype = C.c_void_p
n = 5000
pr = libc.malloc(4 * n); pc = libc.malloc(4 * n)
a1 = (np.arange(n) %% 100).astype(np.int32); a2 = (np.arange(n) * 7 %% 50).astype(np.int32)   # named: alive during memmove
C.memmove(pr, a1.ctypes.data, 4 * n)
C.memmove(pc, a2.ctypes.data, 4 * n)
L.new_sbm.restype = C.POINTER(H.SBM)
L.new_sbm.argtypes = [C.c_long, C.c_long, C.c_long, C.c_void_p, C.c_void_p]
S_ = L.new_sbm(100, 50, n, pr, pc)
y1 = np.empty(100); y2 = np.empty(50)
L.A_mul_B.restype = None; L.At_mul_B.restype = None
o50 = np.ones(50); o100 = np.ones(100)
L.A_mul_B(H._dp(y1), S_, H._dp(o50)); L.At_mul_B(H._dp(y2), S_, H._dp(o100))
assert y1.sum() == n and y2.sum() == n and L.fs_cache_entries() == 2
L.free_sbm.restype = None
L.free_sbm(S_)
assert L.fs_cache_entries() == 0
print("OK")
''' % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FS_STRICT_CACHE="1", FS_DROPIN_MAX_ENTRIES="3")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def test_two_host_threads_share_matrices(hip):
    """bench_a_mul_b.c:401-421 ("[2x cg2]"): two host threads run bsbm_A_mul_B2 on shared B and Bt with their own X / Y,
    while a third keeps invalidating and re-uploading another view of the same matrix: entries are ref-counted, products
    of one handle are serialised by its lock, and every result equals the single-threaded one bit for bit (integer X)"""
    import ctypes as C
    import threading
    be = hip.HipDropinBackend()
    L = be.L
    c = BY_NAME["syn_u16_2048"]
    s = be.sbm(c.nrow, c.ncol, c.rows, c.cols)
    st = be.sbm(c.ncol, c.nrow, c.cols, c.rows)
    B, Bt = L.new_bsbm(C.byref(s), 64), L.new_bsbm(C.byref(st), 64)
    for f in (L.bsbm_A_mul_B2, L.A_mul_B):
        f.restype = None
    blk = O.coo_to_blocked(c.nrow, 64, c.rows, c.cols)
    blkt = O.coo_to_blocked(c.ncol, 64, c.cols, c.rows)
    errors = []

    def worker(seed):
        try:
            X = np.ascontiguousarray(np.stack([S.x_int(seed, c.ncol), S.x_int(seed + 1, c.ncol)], 1))
            Y = np.full((c.nrow, 2), -1.0)
            X2 = np.full((c.ncol, 2), -1.0)
            Yref = O.blocked_mul_n(c.nrow, blk, X, 2)
            X2ref = O.blocked_mul_n(c.ncol, blkt, Yref, 2)
            for _ in range(25):
                L.bsbm_A_mul_B2(hip._dp(Y.reshape(-1)), B, hip._dp(X.reshape(-1)))
                L.bsbm_A_mul_B2(hip._dp(X2.reshape(-1)), Bt, hip._dp(Y.reshape(-1)))
                if not (np.array_equal(Y, Yref) and np.array_equal(X2, X2ref)):
                    errors.append("thread %d: wrong result" % seed)
                    return
        except Exception as ex:       # pragma: no cover
            errors.append(repr(ex))

    stop = threading.Event()

    def churn():
        x = S.x_int(3, c.ncol)
        y = np.full(c.nrow, -1.0)
        ref = O.coo_mul(c.nrow, c.rows, c.cols, None, x)
        while not stop.is_set():
            L.A_mul_B(hip._dp(y), C.byref(s), hip._dp(x))
            if not np.array_equal(y, ref):
                errors.append("churn: wrong result")
                return
            L.fs_invalidate(C.byref(s))

    ts = [threading.Thread(target=worker, args=(10,)), threading.Thread(target=worker, args=(20,)), threading.Thread(target=churn)]
    for t in ts:
        t.start()
    for t in ts[:2]:
        t.join()
    stop.set()
    ts[2].join()
    L.fs_release_all()
    assert not errors, errors


def test_inconsistent_arrays_are_refused_at_creation(hip):
    """the reference validates nothing (a bad index is a host segfault there); on the GPU it would be a memory fault,
    so every matrix is checked once at creation: out-of-range columns / rows and a broken row_ptr give an error, not a
    launch"""
    import torch
    from libfastsparse_amd import capi
    rp = np.array([0, 2, 4], np.int32)
    cc = np.array([0, 1, 2, 3], np.int32)
    for bad_rp, bad_cc, ncol in ((rp, np.array([0, 1, 2, 4], np.int32), 4), (rp, np.array([0, -1, 2, 3], np.int32), 4),
                                 (np.array([0, 3, 2], np.int32), cc, 4), (np.array([1, 2, 4], np.int32), cc, 4),
                                 (np.array([0, 2, 5], np.int32), cc, 4)):
        with pytest.raises(capi.FastsparseError, match="inconsistent"):
            capi.Matrix.from_csr(2, ncol, bad_rp, bad_cc, None)
    with pytest.raises(capi.FastsparseError, match="inconsistent"):
        capi.Matrix.from_coo(2, 4, np.array([0, 2], np.int32), np.array([0, 1], np.int32), None)
    with pytest.raises(capi.FastsparseError, match="inconsistent"):
        capi.Matrix.from_coo(2, 4, torch.tensor([0, 1], dtype=torch.int32, device="cuda"),
                             torch.tensor([0, 7], dtype=torch.int32, device="cuda"), None)
    A = capi.Matrix.from_csr(2, 4, rp, cc, None)      # the consistent one still works
    y = torch.empty(2, dtype=torch.float64, device="cuda")
    A.spmv(y, torch.ones(4, dtype=torch.float64, device="cuda"), capi.current_stream())
    assert y.tolist() == [2.0, 2.0]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_fused_ata_kernel_vs_reference_golden(hip, case):
    """ata_kernel = 2: y = A'A x in ONE kernel (bcsr_AA_mul_B / parallel_bcsr_AA_mul_B, csr.h:305-355) against the
    reference's golden outputs: 1e-12 bar, bit-exact for integer-valued x (small matrices run the CSR form)"""
    from libfastsparse_amd import capi
    gold = np.load(os.path.join(S.GOLDEN, case.name + ".npz"))
    be = hip.HipDeviceBackend()
    capi.set_option("ata_kernel", 2)
    try:
        out = {}
        for tag, x in case.xs.items():
            out["bcsr_AA_mul_B/" + tag] = be.aa_mul(case.nrow, case.ncol, case.rows, case.cols, x, False)
    finally:
        capi.set_option("ata_kernel", 0)
    out = {k: v for k, v in out.items() if k.replace("/", "|") in gold}
    assert out, "no golden bcsr_AA_mul_B output for this case"
    _check(out, gold, case.name, exact=False)


@pytest.mark.parametrize("valued", [False, True])
def test_fused_ata_on_the_lds_staged_copy(hip, valued):
    """the fused kernel's LDS-staged form (t = A x of a row panel kept in LDS, scattered back through the same tiles):
    300 K x 40 K, 48 per row, 586 panels of 512 rows, against the oracle's two serial loops; pattern-only + integer x
    bit for bit; the two-product form gives the same within the bar"""
    import torch
    from libfastsparse_amd import capi
    from oracle import pysynth
    nrow, ncol, per = 300_000, 40_000, 48
    hrp, hcc, hvv = pysynth.uniform(nrow, ncol, per, 0xA7A, valued=valued)
    capi.set_option("ldsx", 2)
    capi.set_option("tile_rows", 512)
    try:
        A = capi.Matrix.from_csr(nrow, ncol, hrp, hcc, hvv)
    finally:
        capi.set_option("ldsx", 1)
        capi.set_option("tile_rows", 0)
    assert A.kernel_name() == "lds-staged"
    rows = np.repeat(np.arange(nrow, dtype=np.int32), per)
    st = capi.current_stream()
    y = torch.full((ncol,), -1.0, dtype=torch.float64, device="cuda")
    tmp = torch.empty(nrow, dtype=torch.float64, device="cuda")
    for x in (S.x_int(8, ncol), S.x_sin(ncol)):
        t_ref = O.csr_mul(nrow, hrp, hcc, hvv, x)
        ref = O.coo_tmul(ncol, rows, hcc, hvv, t_ref)
        absx = O.csr_mul(nrow, hrp, hcc, None if hvv is None else np.abs(hvv), np.abs(x))
        scale = O.coo_tmul(ncol, rows, hcc, None if hvv is None else np.abs(hvv), absx)
        for mode in (2, 0):
            capi.set_option("ata_kernel", mode)
            try:
                A.ata(y, torch.from_numpy(x).cuda(), tmp, st)
            finally:
                capi.set_option("ata_kernel", 0)
            got = y.cpu().numpy()
            if not valued and np.all(x == np.round(x)):
                assert np.array_equal(got, ref), mode
            else:
                assert np.all(np.abs(got - ref) <= TOL * np.maximum(scale, 1e-300)), mode


def test_device_constructors_match_oracle(hip):
    """new_csr / new_bcsr / new_cbcsr / new_bsbm / new_bsdm building on the device (option device_build = 2:
    upload, stable radix sort by row / cell / row block, download) give the reference's arrays element for element
    (the oracle's constructors are pinned to the reference's, tests/test_oracle_vs_ref.py) -- every golden case plus a
    5 M-entry matrix with empty rows, duplicates and a long row, which also takes the device path by default"""
    import ctypes as C
    from libfastsparse_amd import capi
    F = hip.HostFormats()
    big_r, big_c, big_v = S.synth_coo(0xB16, 300_000, 200_000, 17, empty_frac=0.1, dup_frac=0.05, long_row=(7, 40_000))
    cases = [(c.name, c.nrow, c.ncol, c.rows, c.cols, c.vals, c.block_sizes, c.colblocks) for c in CASES]
    cases.append(("mid_300k", 300_000, 200_000, big_r, big_c, big_v, (4096,), (65_536,)))
    for name, nrow, ncol, rows, cols, vals, block_sizes, colblocks in cases:
        rows, cols = np.ascontiguousarray(rows), np.ascontiguousarray(cols)
        v = np.ascontiguousarray(vals) if vals is not None else np.sin(np.arange(len(rows), dtype=np.float64))
        for mode in ((2,) if name != "mid_300k" else (2, 1)):
            capi.set_option("device_build", mode)
            try:
                assert capi.lib().fs_device_build_wanted(len(rows)) == 1, (name, mode)
                A = F.csr(nrow, ncol, rows, cols, v)
                B = F.bcsr(nrow, ncol, rows, cols)
                rp, cc, vv = O.coo_to_csr(nrow, rows, cols, v)
                n = len(rows)
                assert np.array_equal(F.arr(A.row_ptr, nrow + 1, np.int32), rp) and np.array_equal(F.arr(A.cols, n, np.int32), cc)
                assert np.array_equal(F.arr(A.vals, n, np.float64), vv), name
                assert np.array_equal(F.arr(B.row_ptr, nrow + 1, np.int32), rp) and np.array_equal(F.arr(B.cols, n, np.int32), cc)
                for cbs in colblocks:
                    K = F.cbcsr(cbs, nrow, ncol, rows, cols)
                    nb, krp, kcc = O.coo_to_cbcsr(cbs, nrow, ncol, rows, cols)
                    assert K.nblocks == nb and np.array_equal(F.arr(K.row_ptr, nb * nrow + 1, np.int32), krp), (name, cbs)
                    assert np.array_equal(F.arr(K.cols, n, np.int32), kcc), (name, cbs)
                for bs in block_sizes:
                    s_ = F.sdm(nrow, ncol, rows, cols, v)
                    Bd = F.L.new_bsdm(C.byref(s_), bs).contents
                    blk = O.coo_to_blocked(nrow, bs, rows, cols, v)
                    assert Bd.nblocks == blk["nblocks"]
                    assert np.array_equal(F.arr(Bd.start_row, Bd.nblocks + 1, np.int32), blk["start_row"])
                    assert np.array_equal(F.arr(Bd.nnz, Bd.nblocks, np.int32), blk["blk_nnz"])
                    for b in range(0, Bd.nblocks, max(1, Bd.nblocks // 50)):
                        a, e = int(blk["blk_off"][b]), int(blk["blk_off"][b + 1])
                        assert np.array_equal(F.arr(Bd.rows[b], e - a, np.int32), blk["rows"][a:e]), (name, bs, b)
                        assert np.array_equal(F.arr(Bd.cols[b], e - a, np.int32), blk["cols"][a:e])
                        assert np.array_equal(F.arr(Bd.vals[b], e - a, np.float64), blk["vals"][a:e])
            finally:
                capi.set_option("device_build", -1)


def _dist_download(L, ptr, n):
    out = np.empty(n)
    assert L.fs_copy_to_host(out.ctypes.data, ptr, 8 * n) == 0
    return out


def _normal_residual(nrow, ncol, rp, cc, rows_all, lam, xs, b):
    """||b - (A'A + lam I) xs|| / ||b|| with the ORACLE's products (cg.h:9-22): what a solve really left behind"""
    q = O.coo_tmul(ncol, rows_all, cc, None, O.csr_mul(nrow, rp, cc, None, xs)) + lam * xs
    return float(np.linalg.norm(b - q) / np.linalg.norm(b))


def _dist_cg_checks(L, M, ranks, nrow, ncol, rp, cc, rows_all):
    """fs_dist_cg (bsbm_cg, cg.h:25-82, across the ranks) against the oracle's solver.  Three separate questions, each with
    its own numbers in the failure message (round 3 folded them into one assert and lost two of the three):

    (a) an ILL-conditioned system (lambda = 3 under rows of 50 000 ones: ~1 100 iterations).  The iteration count of such a
        solve depends on rounding (any other summation order moves it by several per cent; the reference's own fast-math build
        differs from its strict build the same way), so it is only sanity-bounded; what is REQUIRED is what the caller gets:
        the true relative residual, recomputed with the oracle's products, within 2 x tol -- the recursive residual the
        solver tests (cg.h:69) drifts from the true one by far less at this conditioning -- and the solution within the
        bound the two residuals imply, ||xs - xref|| <= (res_s + res_ref) ||b|| / lambda (A'A + lambda I >= lambda I);
    (b) a WELL-conditioned system (lambda = 3e3: about 45 iterations): there the count must agree within one (the bar of the
        reference goldens, _check above), same residual and solution bounds;
    (c) fixed-order sums (option "reproducible"): two solves give the same count and the same bits."""
    import ctypes as C
    from libfastsparse_amd import capi
    bvec = np.sin(0.37 * np.arange(ncol) + 1.0)
    bnorm = float(np.linalg.norm(bvec))

    def solve(lam, tol):
        xs = np.full(ncol, -1.0)
        it = C.c_int(-1)
        assert L.fs_dist_cg(M, xs.ctypes.data, bvec.ctypes.data, lam, tol, C.byref(it)) == 0, L.fs_last_error()
        return xs, it.value

    # (a)
    lam, tol = 3.0, 1e-8
    xs, it = solve(lam, tol)
    xref, itref = O.cg_normal(nrow, ncol, rows_all, cc, bvec, lam, tol)
    res_s = _normal_residual(nrow, ncol, rp, cc, rows_all, lam, xs, bvec)
    res_ref = _normal_residual(nrow, ncol, rp, cc, rows_all, lam, xref, bvec)
    err2 = float(np.linalg.norm(xs - xref))
    errinf = float(np.max(np.abs(xs - xref)))
    report = dict(ranks=ranks, iterations=it, oracle_iterations=itref, residual=res_s, oracle_residual=res_ref, err2=err2,
                  errinf=errinf, err2_bound=(res_s + res_ref) * bnorm / lam, xmax=float(np.abs(xref).max()))
    print("fs_dist_cg ill-conditioned:", report)
    assert res_ref <= 2 * tol, report                       # (the oracle's own solve, for scale)
    assert res_s <= 2 * tol, report
    assert err2 <= 1.01 * (res_s + res_ref) * bnorm / lam, report
    assert 0.5 * itref <= it <= 1.5 * itref + 2, report
    # (b)
    lam2, tol2 = 3.0e3, 1e-10
    xs2, it2 = solve(lam2, tol2)
    xref2, itref2 = O.cg_normal(nrow, ncol, rows_all, cc, bvec, lam2, tol2)
    res2 = _normal_residual(nrow, ncol, rp, cc, rows_all, lam2, xs2, bvec)
    res2_ref = _normal_residual(nrow, ncol, rp, cc, rows_all, lam2, xref2, bvec)
    report2 = dict(ranks=ranks, iterations=it2, oracle_iterations=itref2, residual=res2, oracle_residual=res2_ref,
                   err2=float(np.linalg.norm(xs2 - xref2)), err2_bound=(res2 + res2_ref) * bnorm / lam2,
                   xmax=float(np.abs(xref2).max()))
    print("fs_dist_cg well-conditioned:", report2)
    assert abs(it2 - itref2) <= 1, report2
    assert res2 <= 2 * tol2 and res2_ref <= 2 * tol2, report2
    assert report2["err2"] <= 1.01 * report2["err2_bound"], report2
    # (c)
    capi.set_option("reproducible", 1)
    try:
        xa, ita = solve(lam, tol)
        xb, itb = solve(lam, tol)
    finally:
        capi.set_option("reproducible", 0)
    res_a = _normal_residual(nrow, ncol, rp, cc, rows_all, lam, xa, bvec)
    report3 = dict(ranks=ranks, iterations=(ita, itb), residual=res_a, differing=int(np.count_nonzero(xa != xb)),
                   maxdiff=float(np.max(np.abs(xa - xb))))
    print("fs_dist_cg fixed-order:", report3)
    assert ita == itb and np.array_equal(xa, xb), report3
    assert res_a <= 2 * tol, report3


@pytest.mark.parametrize("ranks", [1, 3])
def test_native_multi_gpu_context_shards_by_nonzeros(hip, ranks):
    """fs_dist_* (one process, N devices, RCCL): on this one-GPU box the ranks are virtual (device 0 listed N times,
    shards exchanged by device copies -- RCCL refuses duplicate devices), which exercises everything but the collective:
    the nnz-balanced cut of a power-law matrix, local row_ptr per shard, the products, the assembly of y on every rank"""
    import ctypes as C
    from libfastsparse_amd import capi
    from oracle import pysynth
    L = capi.lib()
    nrow = ncol = 200_000
    rp, cc, vv = pysynth.powerlaw(nrow, ncol, 2.3, 50_000, 0xD157)
    devs = (C.c_int * ranks)(*([0] * ranks))
    D = L.fs_dist_create(ranks, devs)
    assert D and L.fs_dist_ndev(D) == ranks and L.fs_dist_uses_rccl(D) == 0
    # shards of 2 M non-zeros would stay on the chunk-streaming kernel (one part): keep the two-pass copy, so that the products
    # really run in FS_DIST_PARTS parts with unequal, padded counts per rank
    capi.set_option("binning", 2)
    try:
        for vals, x in ((vv, S.x_sin(ncol)), (None, S.x_int(5, ncol))):
            M = L.fs_dist_csr_create(D, nrow, ncol, len(cc), rp.ctypes.data, cc.ctypes.data, None if vals is None else vals.ctypes.data)
            assert M, L.fs_last_error()
            b = (C.c_int * (ranks + 1))()
            assert L.fs_dist_matrix_bounds(M, b) == 0
            b = list(b)
            assert b[0] == 0 and b[-1] == nrow and all(b[i] <= b[i + 1] for i in range(ranks))
            per = [int(rp[b[i + 1]] - rp[b[i]]) for i in range(ranks)]
            assert per == [L.fs_dist_matrix_shard_nnz(M, r) for r in range(ranks)]
            assert max(per) - min(per) <= 2 * int(np.diff(rp).max())
            y = np.full(nrow, -1.0)
            assert L.fs_dist_spmv(M, y.ctypes.data, x.ctypes.data) == 0, L.fs_last_error()
            ref = O.csr_mul(nrow, rp, cc, vals, x)
            if vals is None:
                assert np.array_equal(y, ref)
            else:
                assert np.all(np.abs(y - ref) <= TOL * np.maximum(O.csr_abs_scale(nrow, rp, cc, vals, x), 1e-300))
            for r in range(ranks):       # every rank holds the whole y
                assert np.array_equal(_dist_download(L, L.fs_dist_y(M, r), nrow), y), r
            # z = A' u on row shards of A' built from the same host arrays: host vectors ...
            assert L.fs_dist_matrix_has_transpose(M) == 0
            assert L.fs_dist_matrix_build_transpose(M, rp.ctypes.data, cc.ctypes.data, None if vals is None else vals.ctypes.data) == 0, \
                L.fs_last_error()
            assert L.fs_dist_matrix_has_transpose(M) == 1
            u = S.x_int(6, nrow) if vals is None else np.sin(11.0 * np.arange(nrow) - 0.2)
            z = np.full(ncol, -1.0)
            assert L.fs_dist_spmv_t(M, z.ctypes.data, u.ctypes.data) == 0, L.fs_last_error()
            rows_all = np.repeat(np.arange(nrow, dtype=np.int32), np.diff(rp))
            zref = O.coo_tmul(ncol, rows_all, cc, vals, u)
            if vals is None:
                assert np.array_equal(z, zref)
            else:
                assert np.all(np.abs(z - zref) <= TOL * np.maximum(O.coo_tmul(ncol, rows_all, cc, np.abs(vals), np.abs(u)), 1e-300))
            # ... and resident, iterating: x uploaded ONCE, then y = A x, z = A' y, y -> x (square), again; nothing crosses PCIe
            for r in range(ranks):
                assert L.fs_copy_to_device(L.fs_dist_x(M, r), x.ctypes.data, 8 * ncol) == 0
            xi = x.copy()
            for _ in range(2):
                assert L.fs_dist_spmv_resident(M) == 0, L.fs_last_error()
                assert L.fs_dist_spmv_t_resident(M) == 0, L.fs_last_error()
                yi = O.csr_mul(nrow, rp, cc, vals, xi)
                zi = O.coo_tmul(ncol, rows_all, cc, vals, yi)
                for r in range(ranks):
                    gy, gz = _dist_download(L, L.fs_dist_y(M, r), nrow), _dist_download(L, L.fs_dist_z(M, r), ncol)
                    if vals is None:
                        assert np.array_equal(gy, yi) and np.array_equal(gz, zi), r
                    else:
                        assert np.allclose(gy, yi, rtol=1e-10, atol=1e-9 * np.abs(yi).max()) and \
                            np.allclose(gz, zi, rtol=1e-10, atol=1e-9 * np.abs(zi).max()), r
                assert L.fs_dist_swap_xy(M) == 0            # y is the next x
                xi = yi if vals is not None else np.mod(yi, 1024.0)     # keep the integers small: take them mod 1024 on the host ...
                if vals is None:                                           # ... and put that x on every rank
                    for r in range(ranks):
                        assert L.fs_copy_to_device(L.fs_dist_x(M, r), xi.ctypes.data, 8 * ncol) == 0
            # bsbm_cg across the ranks, resident (pattern-only like the reference's BlockedSBM): against the oracle's solver
            if vals is None:
                _dist_cg_checks(L, M, ranks, nrow, ncol, rp, cc, rows_all)
                for r in range(ranks):                       # fs_dist_cg uses x, y and z of the handle as its work vectors
                    assert L.fs_copy_to_device(L.fs_dist_x(M, r), x.ctypes.data, 8 * ncol) == 0
            # a kernel choice that moved after the plan was made (strict_order: the chunk-streaming kernel, one part) is followed
            capi.set_option("strict_order", 1)
            try:
                y2 = np.full(nrow, -1.0)
                assert L.fs_dist_spmv(M, y2.ctypes.data, x.ctypes.data) == 0, L.fs_last_error()
                assert np.array_equal(y2, ref)
            finally:
                capi.set_option("strict_order", 0)
            assert L.fs_dist_spmv(M, y2.ctypes.data, x.ctypes.data) == 0, L.fs_last_error()
            assert np.array_equal(y2, y) or vals is not None        # (valued: the two-pass sums are not run-to-run identical)
            L.fs_dist_matrix_destroy(M)
    finally:
        capi.set_option("binning", 1)
        L.fs_dist_destroy(D)


def test_dropin_csr_A_mul_B_across_ranks_and_rccl_on_one_device(hip):
    """(1) FASTSPARSE_NGPU=3 FASTSPARSE_DEVICES=0,0,0: an unmodified caller of csr_A_mul_B / bcsr_A_mul_B gets the sharded
    product.  (2) FS_DIST_FORCE_RCCL=1 with one device: librccl.so is dlopen'ed, a communicator is created and the all-gather
    runs as a group call on the rank's stream -- the RCCL code path, as far as one GPU can take it."""
    import subprocess
    import sys
    code = r'''
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import _hipbackend as H
from libfastsparse_amd import capi
from oracle import pyoracle as O, pysynth
L = capi.lib()
nrow, ncol = 120_000, 90_000
rp, cc, vv = pysynth.powerlaw(nrow, ncol, 2.3, 20_000, 77)
x = np.sin(7.0 * np.arange(ncol) + 0.3)
xi = (np.arange(ncol) %% 13 - 6).astype(np.float64)
mode = sys.argv[1]
if mode == "dropin":
    A = H.CSR(nrow, ncol, len(cc), H._ip(rp), H._ip(cc), H._dp(vv))
    B = H.BCSR(nrow, ncol, len(cc), H._ip(rp), H._ip(cc))
    y = np.full(nrow, -1.0)
    L.csr_A_mul_B.restype = None; L.bcsr_A_mul_B.restype = None
    L.csr_A_mul_B(H._dp(y), C.byref(A), H._dp(x))
    assert np.all(np.abs(y - O.csr_mul(nrow, rp, cc, vv, x)) <= 1e-12 * np.maximum(O.csr_abs_scale(nrow, rp, cc, vv, x), 1e-300))
    L.bcsr_A_mul_B(H._dp(y), C.byref(B), H._dp(xi))
    assert np.array_equal(y, O.csr_mul(nrow, rp, cc, None, xi))
    # the transposed entry points honour FASTSPARSE_NGPU too (row shards of A' + all-gather)
    L.csr_At_mul_B.restype = None; L.bcsr_At_mul_B.restype = None
    rows_all = np.repeat(np.arange(nrow, dtype=np.int32), np.diff(rp))
    ui = (np.arange(nrow) %% 11 - 5).astype(np.float64)
    z = np.full(ncol, -1.0)
    L.bcsr_At_mul_B(H._dp(z), C.byref(B), H._dp(ui))
    assert np.array_equal(z, O.coo_tmul(ncol, rows_all, cc, None, ui))
    us = np.sin(11.0 * np.arange(nrow) - 0.2)
    L.csr_At_mul_B(H._dp(z), C.byref(A), H._dp(us))
    zr = O.coo_tmul(ncol, rows_all, cc, vv, us)
    assert np.all(np.abs(z - zr) <= 1e-12 * np.maximum(O.coo_tmul(ncol, rows_all, cc, np.abs(vv), np.abs(us)), 1e-300))
    L.fs_release_all()
else:
    D = L.fs_dist_create(1, None)
    assert D and L.fs_dist_uses_rccl(D) == 1, L.fs_last_error()
    M = L.fs_dist_csr_create(D, nrow, ncol, len(cc), rp.ctypes.data, cc.ctypes.data, None)
    y = np.full(nrow, -1.0)
    assert L.fs_dist_spmv(M, y.ctypes.data, xi.ctypes.data) == 0, L.fs_last_error()
    assert np.array_equal(y, O.csr_mul(nrow, rp, cc, None, xi))
    assert L.fs_dist_matrix_build_transpose(M, rp.ctypes.data, cc.ctypes.data, None) == 0, L.fs_last_error()
    ui = (np.arange(nrow) %% 11 - 5).astype(np.float64)
    z = np.full(ncol, -1.0)
    assert L.fs_dist_spmv_t(M, z.ctypes.data, ui.ctypes.data) == 0, L.fs_last_error()
    assert np.array_equal(z, O.coo_tmul(ncol, np.repeat(np.arange(nrow, dtype=np.int32), np.diff(rp)), cc, None, ui))
    L.fs_dist_matrix_destroy(M); L.fs_dist_destroy(D)
print("OK")
''' % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    for mode, extra in (("dropin", {"FASTSPARSE_NGPU": "3", "FASTSPARSE_DEVICES": "0,0,0"}), ("rccl", {"FS_DIST_FORCE_RCCL": "1"})):
        p = subprocess.run([sys.executable, "-c", code, mode], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "OK" in p.stdout, (mode, p.stdout[-1500:] + p.stderr[-1500:])


@pytest.mark.parametrize("kind", ["two-pass", "lds-staged", "tiled", "stream", "long rows"])
def test_non_finite_x_reaches_exactly_the_rows_that_reference_it(hip, kind):
    """csr.h:430-437 multiplies what it is given: a NaN or an infinity in x[c] must reach exactly the rows with an entry in column c
    -- padding entries, zero slots behind a band of x, clamped addresses and masked lanes of the re-ordered copies must not leak
    it into any other row -- and a -0.0 must stay harmless.  Every kept kernel, valued and pattern-only, single vector and k = 2,
    against the oracle (NaN == NaN, infinities with their sign; finite rows within the row-scaled bound)."""
    import torch
    from libfastsparse_amd import capi
    opt, nrow, ncol, per = {"two-pass": ("binning", 200_000, 150_001, 9), "lds-staged": ("ldsx", 120_000, 6_001, 40),
                            "tiled": ("tiling", 200_000, 300_000, 8), "stream": (None, 30_000, 20_000, 10),
                            "long rows": ("binning", 150_000, 120_000, 6)}[kind]
    rng = np.random.default_rng(len(kind))
    lens = rng.integers(0, 2 * per, nrow)
    if kind == "long rows":
        lens[[7, 70_000]] = [90_000, 40_000]
        capi.set_option("long_rows", 2)
    rp = np.zeros(nrow + 1, np.int64); np.cumsum(lens, out=rp[1:]); rp = rp.astype(np.int32)
    cc = rng.integers(0, ncol, int(rp[-1])).astype(np.int32)
    vv = rng.uniform(-1, 1, int(rp[-1]))
    x = S.x_sin(ncol)
    bad = {"nan": 17, "+inf": ncol // 2, "-0": ncol - 1}
    x[bad["nan"]], x[bad["+inf"]], x[bad["-0"]] = np.nan, np.inf, -0.0
    if opt:
        capi.set_option(opt, 2)
    try:
        st = capi.current_stream()
        for vals in (vv, None):
            A = capi.Matrix.from_csr(nrow, ncol, torch.from_numpy(rp).cuda(), torch.from_numpy(cc).cuda(),
                                     None if vals is None else torch.from_numpy(vals).cuda())
            assert A.kernel_name() == {"long rows": "two-pass"}.get(kind, kind), A.kernel_name()
            ref = O.csr_mul(nrow, rp, cc, vals, x)
            xf = np.where(np.isfinite(x), x, 0.0)
            scale = O.csr_abs_scale(nrow, rp, cc, vals, xf)
            y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
            A.spmv(y, torch.from_numpy(x).cuda(), st)
            got = y.cpu().numpy()
            fin = np.isfinite(ref)
            assert 0 < (~fin).sum() < nrow // 2                                         # some rows are hit, most are not
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref)) \
                and np.array_equal(np.isneginf(got), np.isneginf(ref)), kind
            assert np.all(np.abs(got[fin] - ref[fin]) <= TOL * scale[fin]), kind
            X2 = np.ascontiguousarray(np.stack([x, S.x_sin(ncol, 3.0, 0.5)], 1))        # the second column is clean: it must stay clean
            Y2 = torch.full((nrow, 2), -1.0, dtype=torch.float64, device="cuda")
            A.prepare(2, st)
            A.spmm(Y2, torch.from_numpy(X2).cuda(), 2, st)
            g2 = Y2.cpu().numpy()
            r1 = O.csr_mul(nrow, rp, cc, vals, np.ascontiguousarray(X2[:, 1]))
            assert np.all(np.isfinite(g2[:, 1])) and np.all(np.abs(g2[:, 1] - r1) <= TOL * O.csr_abs_scale(nrow, rp, cc, vals, np.ascontiguousarray(X2[:, 1])))
            assert np.array_equal(np.isnan(g2[:, 0]), np.isnan(ref)) and np.array_equal(np.isinf(g2[:, 0]), np.isinf(ref))
            A.close()
    finally:
        if opt:
            capi.set_option(opt, 1)
        capi.set_option("long_rows", 1)


@pytest.mark.parametrize("shape", ["uniform", "uniform_pattern", "holes", "heavy_tail", "small_panels"])
def test_two_pass_copy_with_one_byte_row_ids(hip, shape):
    """where the (band, panel) cells of the two-pass copy are dense -- config 2: 430 entries per cell, in ascending
    row order -- pass 2 reads ONE byte per entry (the step from the entry before it, the row in front of every group of 16 beside it)
    instead of a two-byte row id; a step above 255 is walked by dummy entries of value 0.  Same sums: against the oracle (csr.h:425-438);
    against the two-byte form of the SAME matrix bit for bit where sums are exact (pattern-only, integer x) and within the bar otherwise;
    bit-identical from run to run under `reproducible` (a dummy adds + 0.0); in parts; through the host-vector path."""
    import ctypes as C
    import torch
    from libfastsparse_amd import capi
    L = capi.lib()
    L.fs_debug_two_pass_rows8.restype = C.c_longlong
    L.fs_debug_two_pass_rows8.argtypes = [C.c_void_p, C.c_int]
    rng = np.random.default_rng(20251005)
    opts = {"binning": 2, "ldsx": 0, "tiling": 0}
    if shape in ("uniform", "uniform_pattern"):
        nrow = ncol = 1_000_000
        lens = np.full(nrow, 16)
    elif shape == "holes":                       # one 16 384-row panel with long empty stretches: steps far above 255
        nrow, ncol = 40_000, 5_000
        lens = np.zeros(nrow, np.int64)
        lens[:10_000], lens[16_000], lens[30_000:30_010], lens[39_999] = 3, 2, 5, 1
    elif shape == "heavy_tail":
        nrow, ncol = 60_000, 40_000
        lens = np.minimum((9 / np.maximum(rng.uniform(size=nrow), 1e-6)).astype(np.int64), 50_000) // 8
        opts["long_rows"] = 2
    else:
        nrow, ncol = 5_000, 2_049
        lens = rng.poisson(40, nrow)
        opts["bin_rows"] = 64
    rp = np.zeros(nrow + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rp = rp.astype(np.int32)
    nnz = int(rp[-1])
    cc = rng.integers(0, ncol, nnz).astype(np.int32)
    vv = None if shape == "uniform_pattern" else rng.uniform(-1, 1, nnz)
    st = capi.current_stream()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    xi = rng.integers(-9, 10, ncol).astype(np.float64)
    xs = np.sin(7.0 * np.arange(ncol) + 0.3)
    out = {}
    # arrival-order sums: the same bits only where every sum is exact (pattern-only, integer x); the bar otherwise
    sci = O.csr_abs_scale(nrow, rp, cc, vv, xi)
    same = np.array_equal if vv is None else (lambda a, b: bool(np.all(np.abs(a - b) <= np.maximum(TOL, 2.0 * np.diff(rp) * 2.0 ** -53) * sci)))
    for k, v in opts.items():
        capi.set_option(k, v)
    try:
        for form, flags in (("two_bytes", 64), ("one_byte", 128)):
            capi.set_option("bin_flags", flags)
            A = capi.Matrix.from_csr(nrow, ncol, d(rp), d(cc), None if vv is None else d(vv))
            capi.set_option("bin_flags", 0)
            assert A.kernel_name() == "two-pass"
            dummies = L.fs_debug_two_pass_rows8(A.h, 0)
            assert (dummies == -1) if form == "two_bytes" else (dummies >= 0), (form, dummies)
            if form == "one_byte" and shape == "holes":
                assert dummies >= 20, dummies
            y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
            res = {}
            for name, x in (("int", xi), ("sin", xs)):
                y.fill_(-1.0)
                A.spmv(y, d(x), st)
                res[name] = y.cpu().numpy()
                ref, sc = O.csr_mul(nrow, rp, cc, vv, x), O.csr_abs_scale(nrow, rp, cc, vv, x)
                assert np.all(np.abs(res[name] - ref) <= np.maximum(TOL, 2.0 * np.diff(rp) * 2.0 ** -53) * sc), (form, name)
            capi.set_option("reproducible", 1)
            try:
                y.fill_(-1.0)
                A.spmv(y, d(xs), st)
                res["sin_fixed_order"] = y.cpu().numpy()
                y.fill_(-1.0)
                A.spmv(y, d(xs), st)
                assert np.array_equal(res["sin_fixed_order"], y.cpu().numpy())
            finally:
                capi.set_option("reproducible", 0)
            # in three parts, rows range by range (fs_spmv_part: what the multi-GPU layer ships part by part)
            y.fill_(-1.0)
            for part in range(3):
                A.spmv_part(y, d(xi), part, 3, st)
            assert same(y.cpu().numpy(), res["int"]), form
            # host vectors through the pipelined path
            yh = np.full(nrow, -1.0)
            A.spmv_host(yh, xi)
            assert same(yh, res["int"]), form
            out[form] = res
            A.close()
            if form == "one_byte" and shape == "uniform_pattern":
                # the FIRST fixed-order product of a handle captured into a graph: no allocation and no wait may happen there, so the
                # one-wave pass 2 decodes the one-byte ids on the fly -- the same ids, the same order, the same bits
                capi.set_option("bin_flags", 128)
                B = capi.Matrix.from_csr(nrow, ncol, d(rp), d(cc), None)
                capi.set_option("bin_flags", 0)
                xd, yg = d(xs), torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                capi.set_option("reproducible", 1)
                try:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        B.spmv(yg, xd, capi.current_stream())
                    g.replay()
                    torch.cuda.synchronize()
                finally:
                    capi.set_option("reproducible", 0)
                assert np.array_equal(yg.cpu().numpy(), res["sin_fixed_order"])
                del g
                B.close()
        assert same(out["one_byte"]["int"], out["two_bytes"]["int"])
        # (each form's fixed order is its own: a dummy shifts the entries behind it to other lanes of the one-wave pass 2)
        scs = O.csr_abs_scale(nrow, rp, cc, vv, xs)
        assert np.all(np.abs(out["one_byte"]["sin_fixed_order"] - out["two_bytes"]["sin_fixed_order"]) <= np.maximum(TOL, 2.0 * np.diff(rp) * 2.0 ** -53) * scs)
        if shape == "uniform":                   # and the builder takes the one-byte form by itself where the cells are dense
            A = capi.Matrix.from_csr(nrow, ncol, d(rp), d(cc), d(vv))
            assert 0 <= L.fs_debug_two_pass_rows8(A.h, 0) <= 0.01 * nnz
            A.close()
    finally:
        capi.set_option("bin_flags", 0)
        for k in opts:
            capi.set_option(k, 1 if k in ("binning", "ldsx", "tiling", "long_rows") else 0)


def test_release_and_restore_of_the_plain_csr(hip):
    """once the builder has kept a re-ordered copy the plain arrays are dead weight.  fs_matrix_release_csr gives
    them back (A and A'): the default products are unchanged, the handle holds its copy alone, everything that reads the plain arrays
    (strict_order, the row kernel of k = 8, a new prepare, download) fails with FS_ERR_RELEASED and a message -- never garbage -- and
    fs_matrix_restore_csr brings them back.  fs_matrix_release_prepared drops the k-column copies."""
    import torch
    from libfastsparse_amd import capi
    n, per = 300_000, 16
    capi.set_option("binning", 2)
    try:
        rp, cc, vv = capi.synth_uniform(n, n, per, 0x5EED77)
        A = capi.Matrix.from_csr(n, n, rp, cc, vv)           # an owned copy of the arrays
        st = capi.current_stream()
        A.build_transpose(st)
        assert A.kernel_name() == "two-pass" and A.kernel_name(True) == "two-pass"
        hrp, hcc, hvv = rp.cpu().numpy(), cc.cpu().numpy(), vv.cpu().numpy()
        x = S.x_sin(n)
        xd = torch.from_numpy(x).cuda()
        ref, scale = O.csr_mul(n, hrp, hcc, hvv, x), O.csr_abs_scale(n, hrp, hcc, hvv, x)
        rows = np.repeat(np.arange(n, dtype=np.int32), per)
        zref, zscale = O.coo_tmul(n, rows, hcc, hvv, x), O.coo_tmul(n, rows, hcc, np.abs(hvv), np.abs(x))
        y = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
        A.prepare(2, st)
        X2 = np.ascontiguousarray(np.stack([x, 3.0 * x], 1))
        Y2 = torch.full((n, 2), -1.0, dtype=torch.float64, device="cuda")
        held0 = A.device_bytes()
        assert held0[0] >= 2 * 12 * n * per and held0[2] > 0
        assert A.release_csr() == 2 and A.release_csr() == 0
        held1 = A.device_bytes()
        assert held1[0] == 0 and held1[1] == held0[1] and held1[2] == held0[2]
        for tr, r, sc in ((False, ref, scale), (True, zref, zscale)):
            y.fill_(-1.0)
            A.spmv(y, xd, st, transposed=tr)
            assert np.all(np.abs(y.cpu().numpy() - r) <= TOL * sc)
        A.spmm(Y2, torch.from_numpy(X2).cuda(), 2, st)                  # the prepared k = 2 sweep needs no plain array
        assert np.all(np.abs(Y2.cpu().numpy()[:, 1] - 3.0 * ref) <= 3.0 * TOL * scale)
        for what in (lambda: A.spmm(torch.empty(n, 8, dtype=torch.float64, device="cuda"), torch.zeros(n, 8, dtype=torch.float64, device="cuda"), 8, st),
                     lambda: A.prepare(4, st), lambda: A.download()):
            with pytest.raises(capi.FastsparseError, match="fs_matrix_release_csr"):
                what()
        capi.set_option("strict_order", 1)
        try:
            with pytest.raises(capi.FastsparseError, match="fs_matrix_release_csr"):
                A.spmv(y, xd, st)
            A.restore_csr(rp, cc, vv)                                    # the same arrays back (copied)
            A.spmv(y, xd, st)
            assert np.array_equal(y.cpu().numpy(), ref)                  # storage order: the oracle's bits
        finally:
            capi.set_option("strict_order", 0)
        assert A.device_bytes()[0] >= 12 * n * per
        assert A.release_prepared(2) >= 1 and A.device_bytes()[2] == 0
        assert A.spmm_plan(2) != "k-column two-pass"
        A.close()
        # option release_csr: creation itself gives the arrays back
        capi.set_option("release_csr", 1)
        try:
            B = capi.Matrix.from_csr(n, n, rp, cc, vv)
            assert B.device_bytes()[0] == 0
            B.spmv(y, xd, st)
            assert np.all(np.abs(y.cpu().numpy() - ref) <= TOL * scale)
            B.close()
            # the option is not for the shards of the multi-GPU layer: its own later work (A' on the devices, a k-column prepare)
            # reads their plain arrays
            import ctypes as C
            L = capi.lib()
            D = L.fs_dist_create(2, (C.c_int * 2)(0, 0))
            M = L.fs_dist_csr_create(D, n, n, len(hcc), hrp.ctypes.data, hcc.ctypes.data, hvv.ctypes.data)
            assert M, L.fs_last_error()
            assert L.fs_dist_matrix_build_transpose_device(M) == 0, L.fs_last_error()
            Yh = np.full((n, 2), -1.0)
            assert L.fs_dist_spmm(M, Yh.ctypes.data, X2.ctypes.data, 2) == 0, L.fs_last_error()
            assert np.all(np.abs(Yh[:, 0] - ref) <= TOL * scale)
            L.fs_dist_matrix_destroy(M); L.fs_dist_destroy(D)
        finally:
            capi.set_option("release_csr", 0)
    finally:
        capi.set_option("binning", 1)


def test_solvers_keep_a_lds_staged_copy_that_cannot_be_ordered(hip):
    """fs_cg / fs_cg2 ask for fixed-order sums by default (cg_fixed_order).  On a matrix whose kept LDS-staged copy could
    NOT be arranged one-row-per-wave (dense rows: 300 entries of a row inside one 2048-entry work item) that wish must not move every
    product of the solve to the chunk-streaming kernel: the copy keeps running, in arrival order, and fs_debug_fixed_order_honoured
    says so.  Option "reproducible" = 1 is a requirement: the product then leaves the copy and two runs agree bit for bit."""
    import ctypes as C
    import torch
    from libfastsparse_amd import capi
    L = capi.lib()
    L.fs_debug_ldsx_orderable.argtypes = [C.c_void_p, C.c_int]
    L.fs_debug_fixed_order_honoured.argtypes = [C.c_void_p, C.c_int]
    nrow, ncol, per = 6000, 2048, 300
    capi.set_option("ldsx", 2)
    try:
        hrp, hcc, _ = pysynth_uniform(nrow, ncol, per)
        d = lambda a: torch.from_numpy(a).cuda()
        A = capi.Matrix.from_csr(nrow, ncol, d(hrp), d(hcc), None)
        rows = np.repeat(np.arange(nrow, dtype=np.int32), per)
        At = capi.Matrix.from_coo(ncol, nrow, d(hcc), d(rows), None)
        if A.kernel_name() != "lds-staged" or L.fs_debug_ldsx_orderable(A.h, 0) != 0:
            pytest.skip("the builder arranged this matrix row-per-wave: nothing to check")
        assert L.fs_debug_fixed_order_honoured(A.h, 0) == 0
        st = capi.current_stream()
        x = S.x_sin(ncol)
        y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
        ref, scale = O.csr_mul(nrow, hrp, hcc, None, x), O.csr_abs_scale(nrow, hrp, hcc, None, x)
        A.spmv(y, d(x), st)
        assert np.all(np.abs(y.cpu().numpy() - ref) <= TOL * scale)
        # the solver: same answer with the wish on and off, and as the oracle's within the bar of the golden CG cases
        b1, _ = _cases.cg_rhs(ncol)
        xref, itref = O.cg_normal(nrow, ncol, rows, hcc, b1, 5.0, 1e-6, False)
        for wish in (1, 0):
            capi.set_option("cg_fixed_order", wish)
            xs = torch.full((ncol,), -1.0, dtype=torch.float64, device="cuda")
            it = C.c_int(-1)
            capi.check(L.fs_cg(A.h, At.h, xs.data_ptr(), d(b1).data_ptr(), 5.0, 1e-6, C.byref(it), st), "fs_cg")
            assert abs(it.value - itref) <= 1 and np.max(np.abs(xs.cpu().numpy() - xref)) <= 1e-5 * np.max(np.abs(xref)), (wish, it.value, itref)
        capi.set_option("cg_fixed_order", 1)
        # the requirement: off the copy, onto a fixed-order kernel
        capi.set_option("reproducible", 1)
        try:
            assert A.kernel_name() == "stream"
            A.spmv(y, d(x), st); y1 = y.clone()
            A.spmv(y, d(x), st)
            assert torch.equal(y, y1) and np.all(np.abs(y.cpu().numpy() - ref) <= TOL * scale)
            # option release_csr (plain arrays back once a copy is kept) must not release what the options' products read: created under
            # `reproducible` this handle's products run on the streaming kernel, so its arrays stay (tools/fuzz_parity.py, FS_REPRODUCIBLE=1)
            capi.set_option("release_csr", 1)
            try:
                B = capi.Matrix.from_csr(nrow, ncol, d(hrp), d(hcc), None)
                assert B.kernel_name() == "stream" and B.device_bytes()[0] > 0
                B.spmv(y, d(x), st)
                assert torch.equal(y, y1)
                B.close()
            finally:
                capi.set_option("release_csr", 0)
        finally:
            capi.set_option("reproducible", 0)
        capi.set_option("release_csr", 1)       # and created WITHOUT the requirement the same matrix does give its arrays back
        try:
            B = capi.Matrix.from_csr(nrow, ncol, d(hrp), d(hcc), None)
            assert B.kernel_name() == "lds-staged" and B.device_bytes()[0] == 0
            B.close()
        finally:
            capi.set_option("release_csr", 0)
    finally:
        capi.set_option("ldsx", 1)
        capi.set_option("cg_fixed_order", 1)


def pysynth_uniform(nrow, ncol, per):
    from oracle import pysynth
    return pysynth.uniform(nrow, ncol, per, 0x5EED55, valued=False)


_NGPU3 = {"FASTSPARSE_NGPU": "3", "FASTSPARSE_DEVICES": "0,0,0"}


@pytest.mark.parametrize("mode", ["golden", "resident", "edges", "golden+threads", "resident+threads"])
def test_every_dropin_entry_point_across_three_ranks(hip, mode):
    """FASTSPARSE_NGPU=3 FASTSPARSE_DEVICES=0,0,0 routes EVERY product entry point of sparse.h / dsparse.h /
    csr.h / cbcsr.h / cg.h through the row-sharded path (fs_dropin.hip "several GPUs" -> fs_dist.hip).  `golden`: all golden cases
    through HipDropinBackend with host vectors, the single-GPU bars (bit-exact for pattern matrices with integer x, 1e-12 row-scaled
    otherwise, y pre-poisoned), every output proven to come from sharded products (fs_debug_dist_products).  `resident`: x / y in
    HBM -- read in place and written by the unpack launch, never staged through the host.  `edges`: no entries, no rows, fewer rows
    than ranks, one column, one long row, a struct edited in place.  `+threads`: the same with FS_DIST_THREADS=1, one issuing thread per
    rank (the experimental remedy for the one-process path's issue overhead).  tests/_dropin_ngpu.py is the child."""
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dropin_ngpu.py")
    env = dict(os.environ, **_NGPU3)
    if mode.endswith("+threads"):
        env["FS_DIST_THREADS"] = "1"
    p = subprocess.run([sys.executable, child, mode], env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), (mode, p.stdout[-3000:] + p.stderr[-3000:])


@pytest.mark.gpu
@pytest.mark.parametrize("valued", [True, False])
def test_products_with_host_vectors_overlap_copies(hip, valued):
    """fs_spmv_host / fs_spmv_t_host (what csr_A_mul_B does with malloc'ed vectors): with a two-pass copy x goes up band
    range by band range and y comes down panel range by panel range around the kernels; with cut rows, or any other
    kept copy, it is copy + product + copy.  Every row against the oracle, y pre-poisoned, both directions."""
    from libfastsparse_amd import capi
    rng = np.random.default_rng(41)
    nrow, ncol = 60_000, 100_000          # 7 bands (the last partial), 120 panels of 500 rows
    for long_row in (False, True):
        lens = rng.integers(0, 61, nrow)
        lens[rng.uniform(size=nrow) < 0.1] = 0
        if long_row:
            lens[777] = 5000               # cut into virtual rows: the two-pass copy is kept but the ranges are not used
        rp = np.zeros(nrow + 1, np.int64)
        np.cumsum(lens, out=rp[1:])
        rp = rp.astype(np.int32)
        nnz = int(rp[-1])
        cc = rng.integers(0, ncol, nnz).astype(np.int32)
        cc[-50:] = ncol - 1
        vv = rng.uniform(-1, 1, nnz) if valued else None
        capi.set_option("binning", 2)
        capi.set_option("bin_rows", 500)
        try:
            A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv)
            A.build_transpose(capi.current_stream())
            assert A.kernel_name() == "two-pass" and A.kernel_name(True) == "two-pass"
            rows = np.repeat(np.arange(nrow, dtype=np.int32), lens)
            for x in (S.x_sin(ncol), S.x_int(4, ncol)):
                y = np.full(nrow, -7.0)
                A.spmv_host(y, x)
                assert capi.lib().fs_debug_last_host_path() == (0 if long_row else 1)
                ref = O.csr_mul(nrow, rp, cc, vv, x)
                if not valued and np.all(x == np.round(x)):
                    assert np.array_equal(y, ref)
                else:
                    scale = O.csr_abs_scale(nrow, rp, cc, vv, x)
                    assert np.all(np.abs(y - ref) <= TOL * np.maximum(scale, 1e-300))
            for u in (S.x_sin(nrow, 11.0, -0.2), S.x_int(5, nrow)):
                z = np.full(ncol, -7.0)
                A.spmv_host(z, u, transposed=True)
                zref = O.coo_tmul(ncol, rows, cc, vv, u)
                if not valued and np.all(u == np.round(u)):
                    assert np.array_equal(z, zref)
                else:
                    zscale = O.coo_tmul(ncol, rows, cc, None if vv is None else np.abs(vv), np.abs(u))
                    assert np.all(np.abs(z - zref) <= TOL * np.maximum(zscale, 1e-300))
            A.close()
        finally:
            capi.set_option("binning", 1)
            capi.set_option("bin_rows", 0)
    # the panel kernels (LDS-staged, L2-tiled): every workgroup owns its rows when no panel is shared and no row is cut,
    # and y comes down in ranges of panels; config 3's density, 400 panels of 1000 rows
    nrow, ncol = 400_000, 100_000
    lens = rng.integers(40, 90, nrow)
    lens[rng.uniform(size=nrow) < 0.05] = 0
    lens[:3] = 0
    lens[-2:] = 0
    lens[5000] = 200
    rp = np.zeros(nrow + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rp = rp.astype(np.int32)
    nnz = int(rp[-1])
    cc = rng.integers(0, ncol, nnz).astype(np.int32)
    vv = rng.uniform(-1, 1, nnz) if valued else None
    xs_, xi_ = S.x_sin(ncol), S.x_int(4, ncol)
    ref_s, ref_i = O.csr_mul(nrow, rp, cc, vv, xs_), O.csr_mul(nrow, rp, cc, vv, xi_)
    sc_s = O.csr_abs_scale(nrow, rp, cc, vv, xs_)
    for opts, name in (({"ldsx": 2, "tiling": 0, "binning": 0, "tile_rows": 1000}, "lds-staged"),
                       ({"ldsx": 0, "tiling": 2, "binning": 0, "tile_rows": 1000}, "tiled")):
        for k, v in opts.items():
            capi.set_option(k, v)
        try:
            A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv)
        finally:
            for k, v in (("ldsx", 1), ("tiling", 1), ("binning", 1), ("tile_rows", 0)):
                capi.set_option(k, v)
        assert A.kernel_name() == name
        y = np.full(nrow, -7.0)
        A.spmv_host(y, xs_)
        assert capi.lib().fs_debug_last_host_path() == 2, name
        assert np.all(np.abs(y - ref_s) <= TOL * np.maximum(sc_s, 1e-300)), name
        y[:] = -7.0
        A.spmv_host(y, xi_)
        if valued:
            assert np.all(np.abs(y - ref_i) <= TOL * np.maximum(O.csr_abs_scale(nrow, rp, cc, vv, xi_), 1e-300)), name
        else:
            assert np.array_equal(y, ref_i), name
        A.close()
    # few, long rows (config 3 transposed in small: 50 k x 1.2 M, 960 per row): chunks share panels and are launched stretch
    # of bands by stretch of bands, so x goes up in ranges with the chunks that need no more than what has landed behind it
    nrow, ncol = 1_200_000, 50_000
    rp = (np.arange(nrow + 1, dtype=np.int64) * 40).astype(np.int32)
    nnz = int(rp[-1])
    cc = rng.integers(0, ncol, nnz).astype(np.int32)
    vv = rng.uniform(-1, 1, nnz) if valued else None
    capi.set_option("ldsx", 2)
    capi.set_option("binning", 0)
    capi.set_option("tiling", 0)
    try:
        A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv)
        A.build_transpose(capi.current_stream())
    finally:
        capi.set_option("ldsx", 1)
        capi.set_option("binning", 1)
        capi.set_option("tiling", 1)
    assert A.kernel_name(True) == "lds-staged"
    rows = np.repeat(np.arange(nrow, dtype=np.int32), 40)
    for u in (S.x_sin(nrow, 11.0, -0.2), S.x_int(5, nrow)):
        z = np.full(ncol, -7.0)
        A.spmv_host(z, u, transposed=True)
        assert capi.lib().fs_debug_last_host_path() == 3
        zref = O.coo_tmul(ncol, rows, cc, vv, u)
        if not valued and np.all(u == np.round(u)):
            assert np.array_equal(z, zref)
        else:
            zscale = O.coo_tmul(ncol, rows, cc, None if vv is None else np.abs(vv), np.abs(u))
            assert np.all(np.abs(z - zref) <= TOL * np.maximum(zscale, 1e-300))
    A.close()
    # a small matrix (chunk-streaming kernel) takes the plain path
    rp, cc, vv = (np.array([0, 2, 2, 3], np.int32), np.array([0, 2, 1], np.int32), np.array([1.5, -2.0, 4.0]))
    A = capi.Matrix.from_csr(3, 3, rp, cc, vv)
    y = np.full(3, -7.0)
    A.spmv_host(y, np.array([1.0, 2.0, 3.0]))
    assert capi.lib().fs_debug_last_host_path() == 0
    assert np.array_equal(y, [1.5 - 6.0, 0.0, 8.0])


@pytest.mark.parametrize("case", ["two-pass", "two-pass cut rows", "tiled"])
def test_parts_and_host_vectors_share_a_copy_s_host_mirrors(hip, case):
    """Products in parts and products with host vectors read the same host mirrors of a copy's tables (first rows of the panels;
    with cut rows the rows' first virtual rows), whichever fetches them first: on one handle the product in 4 parts, then
    fs_spmv_host; on a fresh handle the other way round.  The row cuts are the same list both times and really cut, y of the
    parts is y of fs_spmv_host is the oracle's, bit for bit (pattern-only, integer x), and fs_spmv_host goes the way it always
    did: 1 two-pass in ranges (600 panels of 100 rows, more than the 256 resident), 0 with a cut row, 2 the L2-tiled copy in
    ranges of workgroups (400 panels of 1000 rows)."""
    import torch
    from libfastsparse_amd import capi
    rng = np.random.default_rng(43)
    if case == "tiled":
        nrow, ncol, opts, host_path = 400_000, 100_000, {"ldsx": 0, "tiling": 2, "binning": 0, "tile_rows": 1000}, 2
        lens = rng.integers(40, 90, nrow)
    else:
        nrow, ncol, opts, host_path = 60_000, 100_000, {"binning": 2, "bin_rows": 100}, 0 if "cut" in case else 1
        lens = rng.integers(0, 61, nrow)
        lens[rng.uniform(size=nrow) < 0.1] = 0
        if "cut" in case:
            lens[777] = 5000               # cut into virtual rows: the row cuts of the parts come from vfirst
    rp = np.zeros(nrow + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rp = rp.astype(np.int32)
    cc = rng.integers(0, ncol, int(rp[-1])).astype(np.int32)
    x = S.x_int(4, ncol)
    ref = O.csr_mul(nrow, rp, cc, None, x)
    xd = torch.from_numpy(x).cuda()
    st = capi.current_stream()
    defaults = {"ldsx": 1, "tiling": 1, "binning": 1, "tile_rows": 0, "bin_rows": 0}
    cuts = []
    for parts_first in (True, False):
        for k, v in opts.items():
            capi.set_option(k, v)
        try:
            A = capi.Matrix.from_csr(nrow, ncol, rp, cc, None)
        finally:
            for k in opts:
                capi.set_option(k, defaults[k])
        assert A.kernel_name() == case.split(" cut")[0], A.kernel_name()

        def in_parts():
            rows = A.part_rows(4)
            y = torch.full((nrow,), -7.0, dtype=torch.float64, device="cuda")
            for p in range(4):
                A.spmv_part(y, xd, p, 4, st)
            return rows, y.cpu().numpy()

        def with_host_vectors():
            y = np.full(nrow, -7.0)
            A.spmv_host(y, x)
            return y, capi.lib().fs_debug_last_host_path()

        if parts_first:
            (rows, y_parts), (y_host, path) = in_parts(), with_host_vectors()
        else:
            (y_host, path), (rows, y_parts) = with_host_vectors(), in_parts()
        A.close()
        assert path == host_path, (case, parts_first)
        assert np.array_equal(y_parts, ref) and np.array_equal(y_host, ref) and np.array_equal(y_parts, y_host), (case, parts_first)
        assert rows[0] == 0 and rows[-1] == nrow and sum(b > a for a, b in zip(rows, rows[1:])) >= 2, (case, rows)
        cuts.append(rows)
    assert cuts[0] == cuts[1], (case, cuts)


def _shard_arrays(rp, cc, vv, cuts):
    """per-rank arrays of a CSR cut at the rows `cuts`: local row_ptr, global columns, values"""
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = int(rp[a]), int(rp[b])
        out.append((np.ascontiguousarray(rp[a:b + 1] - rp[a]).astype(np.int32), np.ascontiguousarray(cc[lo:hi]),
                    None if vv is None else np.ascontiguousarray(vv[lo:hi])))
    return out


def _ptr_array(C, arrays):
    return (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


def test_native_multi_gpu_shards_with_an_empty_first_shard(hip):
    """the caller chooses the cuts, so shard 0 may be EMPTY (vals[0] == NULL, shard_nnz[0] == 0) on a valued matrix -- it
    used to be taken for a pattern-only matrix and rejected -- and a shard whose row_ptr does not end at its shard_nnz is refused
    before any device kernel trusts it."""
    import ctypes as C
    from libfastsparse_amd import capi
    L = capi.lib()
    ranks = 3
    nrow, ncol = 9000, 7000
    c = BY_NAME["syn_u16_2048"]
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 9, nrow).astype(np.int32)
    lens[:3000] = 0                                            # rows 0 .. 2999 empty: the first shard holds nothing
    rp = np.zeros(nrow + 1, np.int32); np.cumsum(lens, out=rp[1:])
    cc = rng.integers(0, ncol, int(rp[-1])).astype(np.int32)
    vv = rng.uniform(-1, 1, int(rp[-1]))
    cuts = [0, 3000, 6000, nrow]
    shards = _shard_arrays(rp, cc, vv, cuts)
    assert len(shards[0][1]) == 0
    D = L.fs_dist_create(ranks, (C.c_int * ranks)(0, 0, 0))
    assert D
    try:
        p_rp = _ptr_array(C, [s[0] for s in shards])
        p_cc = (C.c_void_p * ranks)(None, shards[1][1].ctypes.data, shards[2][1].ctypes.data)
        p_vv = (C.c_void_p * ranks)(None, shards[1][2].ctypes.data, shards[2][2].ctypes.data)
        srows = (C.c_int * ranks)(3000, 3000, nrow - 6000)
        snnz = (C.c_int64 * ranks)(*[len(s[1]) for s in shards])
        M = L.fs_dist_csr_create_from_shards(D, nrow, ncol, srows, snnz, p_rp, p_cc, p_vv, capi.FS_HOST)
        assert M, L.fs_last_error()
        x = S.x_sin(ncol)
        y = np.full(nrow, -1.0)
        assert L.fs_dist_spmv(M, y.ctypes.data, x.ctypes.data) == 0, L.fs_last_error()
        ref, sc = O.csr_mul(nrow, rp, cc, vv, x), O.csr_abs_scale(nrow, rp, cc, vv, x)
        assert np.all(np.abs(y - ref) <= TOL * sc) and np.all(y[:3000] == 0.0)
        L.fs_dist_matrix_destroy(M)
        bad = (C.c_int64 * ranks)(0, len(shards[1][1]) + 1, len(shards[2][1]))
        assert not L.fs_dist_csr_create_from_shards(D, nrow, ncol, srows, bad, p_rp, p_cc, p_vv, capi.FS_HOST)
        assert b"shard_nnz" in L.fs_last_error()
    finally:
        L.fs_dist_destroy(D)


@pytest.mark.parametrize("space", ["host", "device"])
def test_native_multi_gpu_matrix_from_per_rank_shards_and_device_transpose(hip, space):
    """the native C path must hold a matrix that only exists as per-rank shards (BASELINE config 5: 3.2 G
    entries, more than one `int row_ptr` can index, csr.h:358-366).  fs_dist_csr_create_from_shards takes one CSR per rank (local
    row_ptr, global columns) from host or device memory; fs_dist_matrix_build_transpose_device builds the row shards of A' from
    the device-resident shards of A -- no whole-matrix host array anywhere.  Three virtual ranks on this one GPU: both must equal
    what fs_dist_csr_create + fs_dist_matrix_build_transpose make of the whole matrix: same cuts of A', the same shard arrays
    entry for entry (every row of A' in ascending A-row order), and products bit-exact for integer x, row-scaled otherwise."""
    import ctypes as C
    from libfastsparse_amd import capi
    from oracle import pysynth
    L = capi.lib()
    ranks = 3
    nrow, ncol = 150_000, 110_000
    rp, cc, vv = pysynth.powerlaw(nrow, ncol, 2.3, 30_000, 0x5A4D)
    rows_all = np.repeat(np.arange(nrow, dtype=np.int32), np.diff(rp))
    devs = (C.c_int * ranks)(*([0] * ranks))
    D = L.fs_dist_create(ranks, devs)
    assert D
    try:
        for vals in (vv, None):
            W = L.fs_dist_csr_create(D, nrow, ncol, len(cc), rp.ctypes.data, cc.ctypes.data, None if vals is None else vals.ctypes.data)
            assert W, L.fs_last_error()
            b = (C.c_int * (ranks + 1))()
            assert L.fs_dist_matrix_bounds(W, b) == 0
            cuts = list(b)
            shards = _shard_arrays(rp, cc, vals, cuts)
            keep = []                                  # device copies stay alive until the matrix is made
            if space == "device":
                import torch
                dev = []
                for s_rp, s_cc, s_vv in shards:
                    t = (torch.from_numpy(s_rp).cuda(), torch.from_numpy(s_cc).cuda(), None if s_vv is None else torch.from_numpy(s_vv).cuda())
                    keep.append(t)
                    dev.append(t)
                torch.cuda.synchronize()
                p_rp = (C.c_void_p * ranks)(*[t[0].data_ptr() for t in dev])
                p_cc = (C.c_void_p * ranks)(*[t[1].data_ptr() for t in dev])
                p_vv = None if vals is None else (C.c_void_p * ranks)(*[t[2].data_ptr() for t in dev])
            else:
                p_rp = _ptr_array(C, [s[0] for s in shards])
                p_cc = _ptr_array(C, [s[1] for s in shards])
                p_vv = None if vals is None else _ptr_array(C, [s[2] for s in shards])
            srows = (C.c_int * ranks)(*[cuts[i + 1] - cuts[i] for i in range(ranks)])
            snnz = (C.c_int64 * ranks)(*[len(s[1]) for s in shards])
            M = L.fs_dist_csr_create_from_shards(D, nrow, ncol, srows, snnz, p_rp, p_cc, p_vv, capi.FS_DEVICE if space == "device" else capi.FS_HOST)
            assert M, L.fs_last_error()
            del keep
            assert L.fs_dist_matrix_nnz(M) == len(cc)
            b2 = (C.c_int * (ranks + 1))()
            assert L.fs_dist_matrix_bounds(M, b2) == 0 and list(b2) == cuts
            # A x
            for x in (S.x_int(9, ncol), S.x_sin(ncol)):
                y, yw = np.full(nrow, -1.0), np.full(nrow, -2.0)
                assert L.fs_dist_spmv(M, y.ctypes.data, x.ctypes.data) == 0, L.fs_last_error()
                assert L.fs_dist_spmv(W, yw.ctypes.data, x.ctypes.data) == 0, L.fs_last_error()
                ref = O.csr_mul(nrow, rp, cc, vals, x)
                if vals is None and np.all(x == np.round(x)):
                    assert np.array_equal(y, ref) and np.array_equal(yw, ref)
                else:
                    sc = np.maximum(O.csr_abs_scale(nrow, rp, cc, vals, x), 1e-300)
                    assert np.all(np.abs(y - ref) <= TOL * sc) and np.all(np.abs(yw - ref) <= TOL * sc)
            # A': device build on the sharded matrix, host build on the whole one
            assert L.fs_dist_matrix_has_transpose(M) == 0
            assert L.fs_dist_matrix_build_transpose_device(M) == 0, L.fs_last_error()
            assert L.fs_dist_matrix_build_transpose_device(M) == 0                      # idempotent
            assert L.fs_dist_matrix_build_transpose(W, rp.ctypes.data, cc.ctypes.data, None if vals is None else vals.ctypes.data) == 0, \
                L.fs_last_error()
            bt, btw = (C.c_int * (ranks + 1))(), (C.c_int * (ranks + 1))()
            assert L.fs_dist_matrix_bounds_t(M, bt) == 0 and L.fs_dist_matrix_bounds_t(W, btw) == 0
            assert list(bt) == list(btw), (list(bt), list(btw))
            for r in range(ranks):                    # the shards of A' entry for entry
                got, want = [], []
                for H_, store in ((M, got), (W, want)):
                    sh = L.fs_dist_matrix_shard(H_, r, 1)
                    assert sh
                    n_r, z_r = L.fs_matrix_nrow(sh), L.fs_matrix_nnz(sh)
                    a_rp, a_cc = np.empty(n_r + 1, np.int32), np.empty(max(z_r, 1), np.int32)
                    a_vv = np.empty(max(z_r, 1)) if vals is not None else None
                    assert L.fs_matrix_download(sh, 0, a_rp.ctypes.data, a_cc.ctypes.data, None if a_vv is None else a_vv.ctypes.data) == 0
                    store.extend([a_rp, a_cc[:z_r], None if a_vv is None else a_vv[:z_r]])
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), r
                assert vals is None or np.array_equal(got[2], want[2]), r
            for u in (S.x_int(6, nrow), np.sin(11.0 * np.arange(nrow) - 0.2)):
                z, zw = np.full(ncol, -1.0), np.full(ncol, -2.0)
                assert L.fs_dist_spmv_t(M, z.ctypes.data, u.ctypes.data) == 0, L.fs_last_error()
                assert L.fs_dist_spmv_t(W, zw.ctypes.data, u.ctypes.data) == 0, L.fs_last_error()
                zref = O.coo_tmul(ncol, rows_all, cc, vals, u)
                if vals is None and np.all(u == np.round(u)):
                    assert np.array_equal(z, zref) and np.array_equal(zw, zref)
                else:
                    sc = np.maximum(O.coo_tmul(ncol, rows_all, cc, None if vals is None else np.abs(vals), np.abs(u)), 1e-300)
                    assert np.all(np.abs(z - zref) <= TOL * sc) and np.all(np.abs(zw - zref) <= TOL * sc)
            L.fs_dist_matrix_destroy(M)
            L.fs_dist_matrix_destroy(W)
    finally:
        L.fs_dist_destroy(D)


def test_native_multi_gpu_cg_with_the_vector_work_divided_by_rows(hip):
    """fs_dist_cg, scheme "gather" (option dist_cg_scheme = 1): every rank keeps its slice of x, r, p, q, the
    partial dots are all-gathered and added in rank order, the new p is all-gathered -- against the replicated scheme and the
    oracle's solver, on three virtual ranks; under fixed-order sums (the solvers' default) two solves are bit-identical."""
    import ctypes as C
    from libfastsparse_amd import capi
    from oracle import pysynth
    L = capi.lib()
    ranks = 3
    nrow, ncol = 90_000, 70_000
    rp, cc, _ = pysynth.powerlaw(nrow, ncol, 2.3, 5_000, 0xC6C6)
    rows_all = np.repeat(np.arange(nrow, dtype=np.int32), np.diff(rp))
    devs = (C.c_int * ranks)(*([0] * ranks))
    D = L.fs_dist_create(ranks, devs)
    assert D
    capi.set_option("binning", 2)          # the two-pass copy on these small shards: products in parts, fixed-order pass 2
    try:
        M = L.fs_dist_csr_create(D, nrow, ncol, len(cc), rp.ctypes.data, cc.ctypes.data, None)
        assert M, L.fs_last_error()
        assert L.fs_dist_matrix_build_transpose_device(M) == 0, L.fs_last_error()
        bvec = np.sin(0.37 * np.arange(ncol) + 1.0)
        bnorm = float(np.linalg.norm(bvec))
        lam, tol = 40.0, 1e-9
        xref, itref = O.cg_normal(nrow, ncol, rows_all, cc, bvec, lam, tol)
        res_ref = _normal_residual(nrow, ncol, rp, cc, rows_all, lam, xref, bvec)
        out = {}
        for scheme in (0, 1):
            capi.set_option("dist_cg_scheme", scheme)
            sols = []
            for _ in range(2):
                xs = np.full(ncol, -1.0)
                it = C.c_int(-1)
                assert L.fs_dist_cg(M, xs.ctypes.data, bvec.ctypes.data, lam, tol, C.byref(it)) == 0, L.fs_last_error()
                sols.append((xs, it.value))
            res = _normal_residual(nrow, ncol, rp, cc, rows_all, lam, sols[0][0], bvec)
            rep = dict(scheme=scheme, iterations=[s[1] for s in sols], oracle_iterations=itref, residual=res, oracle_residual=res_ref,
                       err2=float(np.linalg.norm(sols[0][0] - xref)), err2_bound=(res + res_ref) * bnorm / lam,
                       differing=int(np.count_nonzero(sols[0][0] != sols[1][0])))
            print("fs_dist_cg scheme:", rep)
            assert sols[0][1] == sols[1][1] and np.array_equal(sols[0][0], sols[1][0]), rep      # fixed-order sums: bit-identical
            assert res <= 2 * tol and res_ref <= 2 * tol, rep
            assert rep["err2"] <= 1.01 * rep["err2_bound"], rep
            assert abs(sols[0][1] - itref) <= max(2, itref // 10), rep
            out[scheme] = sols[0]
        # the two schemes add the dots in different orders: same solve to rounding, not bit for bit
        assert np.max(np.abs(out[0][0] - out[1][0])) <= 1e-6 * max(1e-300, float(np.abs(xref).max()))
        L.fs_dist_matrix_destroy(M)
    finally:
        capi.set_option("dist_cg_scheme", 0)
        capi.set_option("binning", 1)
        L.fs_dist_destroy(D)


def test_native_multi_gpu_conservative_exchange_and_fallback(hip):
    """the overlapped exchange (one all-gather per part, padded windows) has never run with more than one RCCL rank,
    so there is a conservative mode -- ONE whole-shard all-gather behind the finished local product: FS_DIST_PARTS=1 selects it, and
    an exchange that fails half-issued in the overlapped mode (injected with FS_DIST_FAIL_PART: the first destination's copies /
    rank 0's call are already enqueued) finishes that product conservatively on VIRTUAL ranks and keeps the context there; with
    RCCL the communicators are aborted and the context returns errors (no second collective on a failed group).  Separate
    processes (the environment is read once)."""
    import subprocess
    import sys
    code = r'''
import ctypes as C, os, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from libfastsparse_amd import capi
from oracle import pyoracle as O, pysynth
L = capi.lib()
ranks = int(sys.argv[1])
nrow, ncol = 300_000, 90_000
rp, cc, vv = pysynth.powerlaw(nrow, ncol, 2.3, 20_000, 78)
xi = (np.arange(ncol) %% 13 - 6).astype(np.float64)
capi.set_option("binning", 2)
capi.set_option("bin_rows", 256)     # many panels: the local products really run in parts
D = L.fs_dist_create(ranks, (C.c_int * ranks)(*([0] * ranks)) if ranks > 1 else None)
assert D, L.fs_last_error()
assert L.fs_dist_uses_rccl(D) == (1 if os.environ.get("FS_DIST_FORCE_RCCL") == "1" else 0)
start = L.fs_dist_is_conservative(D)
assert start == (1 if os.environ.get("FS_DIST_PARTS") == "1" else 0)
M = L.fs_dist_csr_create(D, nrow, ncol, len(cc), rp.ctypes.data, cc.ctypes.data, None)
assert M, L.fs_last_error()
ref = O.csr_mul(nrow, rp, cc, None, xi)
if len(sys.argv) > 2 and sys.argv[2] == "k2first":
    # the k-column exchange inside the product (fs_spmm_part) meets the injected failure: finished conservatively on virtual ranks
    X2 = np.ascontiguousarray(np.stack([xi, 2.0 * xi], 1))
    Y2 = np.full((nrow, 2), -1.0)
    assert L.fs_dist_spmm(M, Y2.ctypes.data, X2.ctypes.data, 2) == 0, L.fs_last_error()
    assert np.array_equal(Y2[:, 0], ref) and np.array_equal(Y2[:, 1], 2.0 * ref)
    assert L.fs_dist_is_conservative(D) == 1
    assert L.fs_dist_spmm(M, Y2.ctypes.data, X2.ctypes.data, 2) == 0 and np.array_equal(Y2[:, 1], 2.0 * ref)
if os.environ.get("FS_DIST_FORCE_RCCL") == "1" and os.environ.get("FS_DIST_FAIL_PART"):
    # RCCL: a group call that failed may have launched the collective on some ranks only -- no second collective on those
    # communicators (ADVICE r4): they are aborted, this product and every later one on the context return the error
    y = np.full(nrow, -1.0)
    assert L.fs_dist_spmv(M, y.ctypes.data, xi.ctypes.data) != 0 and b"aborted" in L.fs_last_error(), L.fs_last_error()
    assert L.fs_dist_spmv(M, y.ctypes.data, xi.ctypes.data) != 0 and b"unusable" in L.fs_last_error(), L.fs_last_error()
    L.fs_dist_matrix_destroy(M); L.fs_dist_destroy(D)
    D2 = L.fs_dist_create(1, None)                      # a new context works
    M2 = L.fs_dist_csr_create(D2, nrow, ncol, len(cc), rp.ctypes.data, cc.ctypes.data, None)
    assert L.fs_dist_spmv(M2, y.ctypes.data, xi.ctypes.data) == 0 and np.array_equal(y, ref), L.fs_last_error()
    L.fs_dist_matrix_destroy(M2); L.fs_dist_destroy(D2)
    print("OK"); sys.exit(0)
for rep in range(3):
    y = np.full(nrow, -1.0)
    assert L.fs_dist_spmv(M, y.ctypes.data, xi.ctypes.data) == 0, L.fs_last_error()
    assert np.array_equal(y, ref), rep
    for r in range(ranks):
        g = np.empty(nrow); assert L.fs_copy_to_host(g.ctypes.data, L.fs_dist_y(M, r), 8 * nrow) == 0
        assert np.array_equal(g, ref), (rep, r)
want = 1 if (os.environ.get("FS_DIST_PARTS") == "1" or os.environ.get("FS_DIST_FAIL_PART")) else 0
assert L.fs_dist_is_conservative(D) == want, (L.fs_dist_is_conservative(D), want)
assert L.fs_dist_matrix_build_transpose_device(M) == 0, L.fs_last_error()
ui = (np.arange(nrow) %% 11 - 5).astype(np.float64)
z = np.full(ncol, -1.0)
assert L.fs_dist_spmv_t(M, z.ctypes.data, ui.ctypes.data) == 0, L.fs_last_error()
assert np.array_equal(z, O.coo_tmul(ncol, np.repeat(np.arange(nrow, dtype=np.int32), np.diff(rp)), cc, None, ui))
L.fs_dist_matrix_destroy(M); L.fs_dist_destroy(D)
print("OK")
''' % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    runs = [("3", {}), ("3", {"FS_DIST_PARTS": "1"}), ("3", {"FS_DIST_FAIL_PART": "1"}),
            ("1", {"FS_DIST_FORCE_RCCL": "1"}), ("1", {"FS_DIST_FORCE_RCCL": "1", "FS_DIST_FAIL_PART": "0"}),
            ("1", {"FS_DIST_FORCE_RCCL": "1", "FS_DIST_PARTS": "1"})]
    for ranks, extra in runs:
        p = subprocess.run([sys.executable, "-c", code, ranks], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "OK" in p.stdout, (ranks, extra, p.stdout[-1500:] + p.stderr[-1500:])
    p = subprocess.run([sys.executable, "-c", code, "3", "k2first"], env=dict(os.environ, FS_DIST_FAIL_PART="1"), capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0 and "OK" in p.stdout, ("k2first", p.stdout[-1500:] + p.stderr[-1500:])


_FAILED_EXCHANGE_CHILD = r'''
import ctypes as C, os, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from libfastsparse_amd import capi
from oracle import pyoracle as O, pysynth
L = capi.lib()
k, transposed, ranks = int(sys.argv[1]), int(sys.argv[2]), 3
nrow, ncol = 196_608, 589_824
for f in (L.fs_debug_dist_parts, L.fs_debug_dist_k_parts):
    f.argtypes = [C.c_void_p, C.c_int]
L.fs_debug_dist_k_vector.argtypes = [C.c_void_p, C.c_int, C.c_int]
L.fs_debug_dist_k_vector.restype = C.c_void_p
rp, cc, _ = pysynth.powerlaw(nrow, ncol, 1.1, 1000, 0xFA11, valued=False)
assert 7.0 <= len(cc) / nrow <= 9.0
rows_all = np.repeat(np.arange(nrow, dtype=np.int32), np.diff(rp))
n_in, n_out = (nrow, ncol) if transposed else (ncol, nrow)
X = np.ascontiguousarray(np.stack([(np.arange(n_in) * (j + 3) %% 13 - 6).astype(np.float64) for j in range(k)], 1))
ref = np.stack([O.coo_tmul(ncol, rows_all, cc, None, np.ascontiguousarray(X[:, j])) if transposed else
                O.csr_mul(nrow, rp, cc, None, np.ascontiguousarray(X[:, j])) for j in range(k)], 1)
capi.set_option("binning", 2)
capi.set_option("bin_rows", 256)     # many panels: the local products really run in parts
D = L.fs_dist_create(ranks, (C.c_int * ranks)(*([0] * ranks)))
assert D, L.fs_last_error()
assert L.fs_dist_uses_rccl(D) == 0 and L.fs_dist_is_conservative(D) == 0
M = L.fs_dist_csr_create(D, nrow, ncol, len(cc), rp.ctypes.data, cc.ctypes.data, None)
assert M, L.fs_last_error()
if transposed:
    assert L.fs_dist_matrix_build_transpose_device(M) == 0, L.fs_last_error()
parts1 = L.fs_debug_dist_parts(M, transposed)
print("parts of the single-vector product on the side:", parts1, flush=True)
if k != 3:
    assert parts1 >= 2, parts1
for rep in range(2):                 # the product that meets the injected failure (the first of the process), then one more
    Y = np.full((n_out, k), -1.0)
    rc = (L.fs_dist_spmm_t if transposed else L.fs_dist_spmm)(M, Y.ctypes.data, X.ctypes.data, k)
    assert rc == 0, L.fs_last_error()
    assert np.array_equal(Y, ref), rep
    for r in range(ranks):
        if k == 1:
            ptr = (L.fs_dist_z if transposed else L.fs_dist_y)(M, r)
        else:
            ptr = L.fs_debug_dist_k_vector(M, r, 2 if transposed else 1)
        g = np.empty((n_out, k)); assert ptr and L.fs_copy_to_host(g.ctypes.data, ptr, 8 * n_out * k) == 0
        assert np.array_equal(g, ref), (rep, r)
    if k > 1:                        # (the k-column plan exists from the first k-column product on: the plan that product ran on)
        kparts = L.fs_debug_dist_k_parts(M, transposed)
        print("parts of the k-column product on the side:", kparts, flush=True)
        assert kparts <= 1 if k == 3 else kparts >= 2, kparts
    # k = 3 finishes no rows in parts: whole-shard mode, the injection never fires, the context stays as it was
    assert L.fs_dist_is_conservative(D) == (0 if k == 3 else 1), rep
L.fs_dist_matrix_destroy(M); L.fs_dist_destroy(D)
print("OK")
''' % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k,side,fail_part", [(1, "A'", "0"), (2, "A'", "1"), (4, "A", "0"), (4, "A'", "last"), (3, "A", "1")])
def test_native_multi_gpu_failed_exchange_every_k_and_side(hip, k, side, fail_part):
    """One engine runs the product of every k on both sides, so every (k, side) meets the injected failure of an exchange
    (FS_DIST_FAIL_PART, virtual ranks) the same way: the remaining parts run, the streams drain, ONE whole-shard gather finishes the
    product and the context stays conservative.  Per case, in a child process of its own (the environment and the injection are
    read once per process), on 3 virtual ranks and a binary power-law matrix with about 8 entries per row (binning 2, bin_rows
    256; integer-valued x, so sums are exact): the product that meets the failure -- the first of the
    process -- is the oracle's bit for bit, so is every rank's resident copy, fs_dist_is_conservative is 1 afterwards, and a
    second product is exact again.  Before the product the side's single-vector product must finish rows in >= 2 parts
    (fs_debug_dist_parts); for k > 1 the k-column plan only exists once the first k-column product made it, so
    fs_debug_dist_k_parts >= 2 is asserted right behind that product, on the plan it ran on.  k = 3 finishes no rows in parts
    (<= 1): the injection must not fire and the context must stay non-conservative.  "last": the last of the FS_DIST_PARTS
    (default 4) parts.

    Shape: 196 608 x 589 824 (grown from 12 288 x 4 096, where every product finished its rows in ONE part).  A two-pass
    product is cut by generations of resident workgroups, so a shard finishes rows in parts only with more panels than the 256 CUs:
    at bin_rows 256 (about 205 rows per panel) more than 52 224 rows -- A's shards hold about 65 000 (2 parts).  Failing the LAST
    of 4 parts needs rows in all 4: more than 768 panels, 157 082 rows -- the shards of A' hold about 196 000."""
    import subprocess
    import sys
    part = str(int(os.environ.get("FS_DIST_PARTS", "4")) - 1) if fail_part == "last" else fail_part
    p = subprocess.run([sys.executable, "-c", _FAILED_EXCHANGE_CHILD, str(k), str(int(side == "A'"))], env=dict(os.environ, FS_DIST_FAIL_PART=part),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, (k, side, fail_part, p.stdout[-1500:] + p.stderr[-1500:])


@pytest.mark.parametrize("valued", [False, True])
def test_lds_staged_kernel_fixed_order_sums(hip, valued):
    """the LDS-staged kernel under fixed-order sums.  A config-3-shaped matrix (tall, dense tiles; binary like
    config 3, and valued) keeps its LDS-staged copy under option "reproducible" -- the builder puts all entries of a row inside a
    work item with ONE wave (fs_debug_ldsx_orderable), the kernel waits for a phase's adds before the phase's barrier, chunks that
    share a panel (the transpose: few, long rows) add their slices in turn -- and then: x = sin, repeated products bit-identical,
    every row within 1e-12 row-scaled of the oracle, both directions; the slices through the registers (x 8 bytes off) as well."""
    import ctypes as C
    import torch
    from libfastsparse_amd import capi
    L = capi.lib()
    nrow, ncol, per = 1_200_000, 200_000, 48
    rp, cc, vv = capi.synth_uniform(nrow, ncol, per, 0x0C3, valued=valued)
    rpn, ccn = rp.cpu().numpy(), cc.cpu().numpy()
    vvn = vv.cpu().numpy() if valued else None
    st = capi.current_stream()
    L.fs_debug_ldsx_orderable.argtypes = [C.c_void_p, C.c_int]
    capi.set_option("ldsx", 2)
    try:
        A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv, borrow=True)
        A.build_transpose(st)
    finally:
        capi.set_option("ldsx", 1)
    assert A.kernel_name() == "lds-staged" and A.kernel_name(True) == "lds-staged"
    assert L.fs_debug_ldsx_orderable(A.h, 0) == 1 and L.fs_debug_ldsx_orderable(A.h, 1) == 1
    rows_all = np.repeat(np.arange(nrow, dtype=np.int32), per)
    xs_ = np.sin(7.0 * np.arange(ncol) + 0.3)
    us_ = np.sin(11.0 * np.arange(nrow) - 0.2)
    ref = O.csr_mul(nrow, rpn, ccn, vvn, xs_)
    sc = np.maximum(O.csr_abs_scale(nrow, rpn, ccn, vvn, xs_), 1e-300)
    reft = O.coo_tmul(ncol, rows_all, ccn, vvn, us_)
    sct = np.maximum(O.coo_tmul(ncol, rows_all, ccn, None if vvn is None else np.abs(vvn), np.abs(us_)), 1e-300)
    xd, ud = torch.from_numpy(xs_).cuda(), torch.from_numpy(us_).cuda()
    xoff = torch.zeros(ncol + 1, dtype=torch.float64, device="cuda")
    xoff[1:] = xd
    y = torch.full((nrow,), -1.0, dtype=torch.float64, device="cuda")
    z = torch.full((ncol,), -1.0, dtype=torch.float64, device="cuda")
    capi.set_option("reproducible", 1)
    try:
        assert A.kernel_name() == "lds-staged" and A.kernel_name(True) == "lds-staged"      # the copy stays
        ys, zs = [], []
        for _ in range(4):
            y.fill_(-1.0); z.fill_(-1.0)
            A.spmv(y, xd, st)
            A.spmv(z, ud, st, transposed=True)
            ys.append(y.cpu().numpy().copy()); zs.append(z.cpu().numpy().copy())
        assert all(np.array_equal(ys[0], v_) for v_ in ys[1:]), "A x differs between runs under fixed-order sums"
        assert all(np.array_equal(zs[0], v_) for v_ in zs[1:]), "A' u differs between runs under fixed-order sums"
        assert np.all(np.abs(ys[0] - ref) <= TOL * sc) and np.all(np.abs(zs[0] - reft) <= TOL * sct)
        # no chunk gave up waiting for its turn and added out of turn (a silent break of the fixed order must show)
        L.fs_debug_ldsx_ticket_giveups.argtypes = [C.c_void_p, C.c_int]
        assert L.fs_debug_ldsx_ticket_giveups(A.h, 0) == 0 and L.fs_debug_ldsx_ticket_giveups(A.h, 1) == 0
        # ... and across BUILDS: a second handle made from the same arrays arranges its work items the same way (the format
        # builder is deterministic), so its fixed-order sums are the first handle's, bit for bit -- what "the same result in every
        # run of the program" needs
        capi.set_option("ldsx", 2)
        try:
            A2 = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv, borrow=True)
            A2.build_transpose(st)
        finally:
            capi.set_option("ldsx", 1)
        y.fill_(-1.0); z.fill_(-1.0)
        A2.spmv(y, xd, st)
        A2.spmv(z, ud, st, transposed=True)
        assert np.array_equal(y.cpu().numpy(), ys[0]) and np.array_equal(z.cpu().numpy(), zs[0]), "a second build adds in another order"
        del A2
        # the form without LDS DMA (x not 16-byte aligned): every phase ends in a full barrier, the same guarantee
        yo = []
        for _ in range(2):
            y.fill_(-1.0)
            A.spmv(y, xoff[1:], st)
            yo.append(y.cpu().numpy().copy())
        assert np.array_equal(yo[0], yo[1]) and np.all(np.abs(yo[0] - ref) <= TOL * sc)
    finally:
        capi.set_option("reproducible", 0)
    y.fill_(-1.0); z.fill_(-1.0)
    A.spmv(y, xd, st)
    A.spmv(z, ud, st, transposed=True)
    assert np.all(np.abs(y.cpu().numpy() - ref) <= TOL * sc) and np.all(np.abs(z.cpu().numpy() - reft) <= TOL * sct)
    # integer x: exact in every mode
    if not valued:
        xi = S.x_int(3, ncol)
        A.spmv(y, torch.from_numpy(xi).cuda(), st)
        assert np.array_equal(y.cpu().numpy(), O.csr_mul(nrow, rpn, ccn, None, xi))


@pytest.mark.parametrize("ranks", [1, 3])
def test_plain_c_caller_of_the_multi_gpu_abi(hip, ranks, tmp_path):
    """north_star: "host C dispatching through a thin C-ABI ... rows range-partitioned across the GPUs".  tests/c/dist_shards_caller.c
    is a C99 program that includes only include/fastsparse_hip.h: per-rank shards in, A' built on the devices, both products
    checked bit for bit against the reference's serial loops restated in it, bsbm_cg across the ranks checked by its residual."""
    import shutil
    import subprocess
    from libfastsparse_amd import capi
    capi.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "libfastsparse_amd")
    exe = str(tmp_path / "dist_shards_caller")
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.run([gcc, "-std=gnu99", "-O2", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "c", "dist_shards_caller.c"),
                    "-o", exe, "-L" + libdir, "-lfastsparse_hip", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    p = subprocess.run([exe, str(ranks)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.startswith("OK ranks=%d" % ranks), (p.stdout[-800:], p.stderr[-800:])


def _ref_caller(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return os.path.join(root, "oracle", "_ref", name)


def _data_dir(tmp_path):
    """the reference's programs open data/sbm-100-50.data and data/sdm-100-50.data relative to their working directory"""
    import shutil
    d = tmp_path / "data"
    d.mkdir()
    for f in ("sbm-100-50.data", "sdm-100-50.data"):
        shutil.copy(os.path.join(S.GOLDEN, f), d / f)
    return str(tmp_path)


def test_the_references_own_test_program_passes_on_the_product_library(hip, tmp_path):
    """The drop-in claim, checked by the reference itself: oracle/_ref/test_sparse_hip is the reference's OWN test program
    (test_sparse.c, compiled in the build container from /root/reference against the reference's ORIGINAL headers at -O0, where C99
    inline leaves every API call an undefined symbol: SURVEY 8b) linked against libfastsparse_hip.so -- `make -C oracle ref-callers`.
    Every product of its 29 tests (A_mul_B, At_mul_B, bcsr_*, bsbm_*, sdm_*, bsdm_*, csr_*, cbcsr_*, the CG solvers' products, the
    loaders and sorters) therefore runs through the product on this GPU.  The binary is test infrastructure; only built where the
    reference is present."""
    import subprocess
    exe = _ref_caller("test_sparse_hip")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/test_sparse_hip was not built (no /root/reference where build() ran)")
    p = subprocess.run([exe], cwd=_data_dir(tmp_path), capture_output=True, text=True, timeout=600)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "ALL TESTS PASSED" in out and "Tests run: 29" in out, out[-2000:]


def test_the_references_own_test_program_passes_across_three_ranks(hip, tmp_path):
    """the same binary with FASTSPARSE_NGPU=3 FASTSPARSE_DEVICES=0,0,0: all 29 of the reference's tests with every product on the
    row-sharded path (three virtual ranks on this GPU); FS_TRACE_DIST=1 makes the library report how many sharded products it ran"""
    import subprocess
    exe = _ref_caller("test_sparse_hip")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/test_sparse_hip was not built (no /root/reference where build() ran)")
    cwd = _data_dir(tmp_path)
    p = subprocess.run([exe], cwd=cwd, env=dict(os.environ, FS_TRACE_DIST="1", **_NGPU3), capture_output=True, text=True,
                       timeout=900)
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "ALL TESTS PASSED" in out and "Tests run: 29" in out, out[-2000:]
    import re
    m = re.search(r"\[fastsparse\] (\d+) sharded products on 3 ranks", out)
    assert m and int(m.group(1)) >= 30, out[-2000:]
    # and the reference's harness, every section, incl. the two host threads of "[2x cg2]" sharing the context
    exe = _ref_caller("bench_a_mul_b_hip")
    if os.path.exists(exe):
        p = subprocess.run([exe, "-f", "data/sbm-100-50.data", "-r", "-c"], cwd=cwd, env=dict(os.environ, **_NGPU3),
                           capture_output=True, text=True, timeout=900)
        out = p.stdout + p.stderr
        assert p.returncode == 0, out[-2000:]
        for label in ("[unsorted]", "[block]", "[cg2]", "[csr]", "[cg8**-csr]", "[BlockCG2]\tniter:", "[2x cg2]"):
            assert label in out, (label, out[-2000:])


def test_the_references_own_bench_harness_runs_on_the_product_library(hip, tmp_path):
    """the reference's benchmark harness (bench_a_mul_b.c from /root/reference, original headers, -O0) linked against the product
    library, on both bundled fixtures with every section switched on (BASELINE configs[0]): exits 0 and prints its section labels"""
    import subprocess
    exe = _ref_caller("bench_a_mul_b_hip")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/bench_a_mul_b_hip was not built (no /root/reference where build() ran)")
    cwd = _data_dir(tmp_path)
    for flags in (["-r", "-c"], ["-r", "-c", "-t"], ["-b", "16"]):
        p = subprocess.run([exe, "-f", "data/sbm-100-50.data"] + flags, cwd=cwd, capture_output=True, text=True, timeout=600)
        out = p.stdout + p.stderr
        assert p.returncode == 0, (flags, out[-2000:])
        labels = ["[unsorted]", "[sort]", "[block]", "[2xblock]", "[cg]", "[cg2]", "[4xblock]", "[sort+block]", "[rowsort+block]",
                  "[2x cg2]"]
        if "-r" in flags:
            labels += ["[csr]", "[csr2]", "[cg2-csr]", "[cg4-csr]", "[cg8-csr]", "[cg8a-csr]", "[cg8*-csr]", "[cg8**-csr]"]
        if "-c" in flags:
            labels += ["[BlockCG2]\tniter:"]
        for label in labels:
            assert label in out, (flags, label, out[-2000:])
    # bench_csr.c: the fused A'A x of parallel_bcsr_AA_mul_B (csr.h:323) on the fixture and on its transpose
    exe = _ref_caller("bench_csr_hip")
    if os.path.exists(exe):
        for flags in ([], ["-t"]):
            p = subprocess.run([exe, "-f", "data/sbm-100-50.data"] + flags, cwd=cwd, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0 and "[par B'B x]" in p.stdout, (flags, (p.stdout + p.stderr)[-2000:])


@pytest.mark.parametrize("ranks", [1, 3])
def test_native_multi_gpu_k_column_products_and_block_cg(hip, ranks):
    """the native multi-GPU path with k row-major columns: fs_dist_spmm / fs_dist_spmm_t (csr_A_mul_Bn, bsbm_A_mul_Bn across the
    ranks) against the oracle -- pattern-only with integer X bit for bit, valued within the row-scaled bar -- and fs_dist_cg2
    (bsbm_cg2, cg.h:85-187, across the ranks) against the oracle's block solver: iteration count within one on a well-conditioned
    system, true residuals of both columns within 2 tol, two solves bit-identical (fixed-order products are the solvers' default)."""
    import ctypes as C
    from libfastsparse_amd import capi
    from oracle import pysynth
    L = capi.lib()
    nrow, ncol = 120_000, 80_000
    rp, cc, vv = pysynth.powerlaw(nrow, ncol, 2.3, 8_000, 0xB10C)
    rows_all = np.repeat(np.arange(nrow, dtype=np.int32), np.diff(rp))
    D = L.fs_dist_create(ranks, (C.c_int * ranks)(*([0] * ranks)))
    assert D
    capi.set_option("binning", 2)
    capi.set_option("bin_rows", 64)        # many panels per shard: the k = 2 sweep finishes its rows in several parts
    L.fs_debug_dist_k_parts.argtypes = [C.c_void_p, C.c_int]
    try:
        for vals in (None, vv):
            M = L.fs_dist_csr_create(D, nrow, ncol, len(cc), rp.ctypes.data, cc.ctypes.data, None if vals is None else vals.ctypes.data)
            assert M, L.fs_last_error()
            assert L.fs_dist_matrix_build_transpose_device(M) == 0, L.fs_last_error()
            for k in (2, 3):
                X = np.ascontiguousarray(np.stack([S.x_int(20 + j, ncol) for j in range(k)], 1)) if vals is None else S.X_sin(ncol, k)
                Y = np.full((nrow, k), -1.0)
                assert L.fs_dist_spmm(M, Y.ctypes.data, X.ctypes.data, k) == 0, L.fs_last_error()
                ref = O.csr_mul_n(nrow, rp, cc, vals, X, k)
                U = np.ascontiguousarray(np.stack([S.x_int(30 + j, nrow) for j in range(k)], 1)) if vals is None else \
                    np.ascontiguousarray(np.stack([np.sin(11.0 * np.arange(nrow) - 0.2 + j) for j in range(k)], 1))
                Z = np.full((ncol, k), -1.0)
                assert L.fs_dist_spmm_t(M, Z.ctypes.data, U.ctypes.data, k) == 0, L.fs_last_error()
                if k == 2 and ranks > 1:        # the exchange ran INSIDE the product (round 5): the sweep was really cut
                    assert L.fs_debug_dist_k_parts(M, 0) >= 2 and L.fs_debug_dist_k_parts(M, 1) >= 2, \
                        (L.fs_debug_dist_k_parts(M, 0), L.fs_debug_dist_k_parts(M, 1))
                for j in range(k):
                    zref = O.coo_tmul(ncol, rows_all, cc, vals, np.ascontiguousarray(U[:, j]))
                    if vals is None:
                        assert np.array_equal(Y[:, j], ref[:, j]) and np.array_equal(Z[:, j], zref), (k, j)
                    else:
                        sy = np.maximum(O.csr_abs_scale(nrow, rp, cc, vals, np.ascontiguousarray(X[:, j])), 1e-300)
                        sz = np.maximum(O.coo_tmul(ncol, rows_all, cc, np.abs(vals), np.abs(np.ascontiguousarray(U[:, j]))), 1e-300)
                        assert np.all(np.abs(Y[:, j] - ref[:, j]) <= TOL * sy) and np.all(np.abs(Z[:, j] - zref) <= TOL * sz), (k, j)
            if vals is None:            # the reference's CG consumers run on pattern matrices (BlockedSBM)
                B = np.ascontiguousarray(np.stack([np.sin(0.37 * np.arange(ncol) + 1.0), np.cos(0.23 * np.arange(ncol) + 0.7)], 1))
                lam, tol = 5000.0, 1e-9          # well-conditioned: the count must agree within one (a 55-iteration solve at lambda =
                Xref, itref = O.cg_normal(nrow, ncol, rows_all, cc, B, lam, tol, two=True)   # 300 moved by 3 with the shard cuts)
                sols = []
                for _ in range(2):
                    Xs = np.full((ncol, 2), -1.0)
                    it = C.c_int(-1)
                    assert L.fs_dist_cg2(M, Xs.ctypes.data, B.ctypes.data, lam, tol, C.byref(it)) == 0, L.fs_last_error()
                    sols.append((Xs, it.value))
                res = [_normal_residual(nrow, ncol, rp, cc, rows_all, lam, np.ascontiguousarray(sols[0][0][:, j]), np.ascontiguousarray(B[:, j]))
                       for j in range(2)]
                rep = dict(ranks=ranks, iterations=[s_[1] for s_ in sols], oracle_iterations=itref, residuals=res,
                           errinf=float(np.max(np.abs(sols[0][0] - Xref))), xmax=float(np.abs(Xref).max()))
                print("fs_dist_cg2:", rep)
                assert sols[0][1] == sols[1][1] and np.array_equal(sols[0][0], sols[1][0]), rep
                assert abs(sols[0][1] - itref) <= 1 and max(res) <= 2 * tol, rep
                assert rep["errinf"] <= 1e-6 * max(1e-300, rep["xmax"]), rep
            L.fs_dist_matrix_destroy(M)
    finally:
        capi.set_option("binning", 1)
        capi.set_option("bin_rows", 0)
        L.fs_dist_destroy(D)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["syn_u16_2048", "syn_long_800x5000", "syn_wide_300x40000"])
def test_copy_geometry_matches_the_plan_model(hip, name):
    """The geometry the device builders really laid out equals what tests/_plan_model.py -- the restatement of fs_plan.h that
    tests/test_format_plans.py holds the C++ to on the CPU -- predicts from the CSR and the device's CU count, on three forced
    paths: the L2-tiled copy with cut rows and small tiles, the LDS-staged copy, the two-pass copy."""
    import ctypes as C
    import torch
    import _plan_model as M
    from libfastsparse_amd import capi
    c = next(k for k in CASES if k.name == name)
    rp, cc, vv = O.coo_to_csr(c.nrow, c.rows, c.cols, c.vals)
    nnz, ncu = int(rp[-1]), torch.cuda.get_device_properties(0).multi_processor_count
    slots = M.tiled_slots(ncu)
    L = capi.lib()
    L.fs_debug_tiled_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.fs_debug_tiled_layout.argtypes = [C.c_void_p, C.c_int]
    L.fs_debug_two_pass_layout.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]

    def build(**opts):
        for k, v in opts.items():
            capi.set_option(k, v)
        try:
            return capi.Matrix.from_csr(c.nrow, c.ncol, rp, cc, vv)
        finally:
            for k in opts:
                capi.set_option(k, 1 if k in ("tiling", "ldsx", "binning") else 0)

    def tiled(A, ldsx, tile_rows, tile_cols, split):
        vp, cut = M.virtual_rows(rp, split) if not ldsx else ([int(v) for v in rp], False)
        nvrow = len(vp) - 1
        R = M.plan_tiled_rows(nvrow, slots, M.K_LDSX_ROWS if ldsx else M.K_TILED_ROWS_MAX, ldsx, tile_rows)
        panel_row = M.plan_tiled_panels(nvrow, R, cut, vp, nnz, split)
        P = len(panel_row) - 1
        W, J = M.plan_band_width(c.ncol, nnz, P, ldsx, tile_cols)
        tp = M.tile_pointers(vp, panel_row, cc, W, J)
        items, item_ptr = M.cut_work_items(tp, P, J)
        shared = bool(ldsx) and M.plan_ldsx_chunks(item_ptr, len(items), P, slots, os.environ.get("FS_LDSX_ORDER", "")[:1] == "1")["shared"] == [1]
        g = (C.c_int * 6)()
        assert L.fs_debug_tiled_geometry(A.h, g) == 0
        print(name, "lds-staged" if ldsx else "tiled", "R W P J nitems", list(g)[:5], "predicted", [R, W, P, J, len(items)], "cut", cut, "shared", shared)
        assert list(g)[:5] == [R, W, P, J, len(items)]
        assert L.fs_debug_tiled_layout(A.h, 0) == (1 if cut else 0) | (2 if shared else 0)
        return cut

    A = build(tiling=2, tile_rows=64, tile_cols=128, tile_split=5)
    assert A.kernel_name() == "tiled"
    assert tiled(A, False, 64, 128, 5) == (np.diff(rp).max() > 5)
    A.close()
    A = build(ldsx=2)
    assert A.kernel_name() == "lds-staged"
    tiled(A, True, 0, 0, 256)
    A.close()
    A = build(binning=2, bin_flags=64)
    assert A.kernel_name() == "two-pass"
    g = M.plan_two_pass_geometry(c.nrow, c.ncol, nnz, 1, 0, int(os.environ.get("FS_BIN_BIG") or -1))
    vp, cut = M.virtual_rows(rp, 256)
    panel_row = M.plan_two_pass_panels(vp, len(vp) - 1, nnz, g["R"], ncu if ncu > 0 else 256, float(os.environ.get("FS_BIN_FILL") or 80) / 100.0,
                                       int(os.environ.get("FS_BIN_MIN_PANELS") or 1), 1)
    lay = (C.c_ulonglong * 8)()
    assert L.fs_debug_two_pass_layout(A.h, 0, lay) == 0
    print(name, "two-pass B P", int(lay[6]), int(lay[7]), "predicted", -(-c.ncol // g["bcols"]), len(panel_row) - 1, "cut", cut)
    assert (int(lay[6]), int(lay[7])) == (-(-c.ncol // g["bcols"]), len(panel_row) - 1)
    assert cut == (name == "syn_long_800x5000")
    A.close()
