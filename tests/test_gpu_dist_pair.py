"""fs_dist_matrix_pair(A, At): a third sharded handle on the shards of two others -- direct side A's, transposed side the caller's own
At -- on every sharded path, on virtual ranks of one device (fs_dist_create(n, [0] * n)), on the harness of tests/_solvers.py and
tests/_dist_solvers.py.  What a pair has that a built transpose has not: rows of A' in the CALLER's entry order (System.t_csr_coo();
a built transpose sorts them), the caller's cuts of A' (empty shards in the middle, one-row shards), sides shared by two handles
each, and a life of its own.  tests/test_dist_pair_model.py shows on the CPU that the models used here tell the two transposes and
the two kinds of cuts apart.

0  PairDist (tests/_dist_solvers.py): Dist's surface on a pair, three routes to A and At; the shards of A' are the caller's arrays, array for array.
1  (on the CPU: tests/test_dist_pair_model.py)
2  products: strict_order bit for bit against the oracle on the caller's A'; the exact sets in the other three modes; arbitrary
   data within 1e-12 row-scaled; the direct side through the pair is the direct side through A.
3  solvers under strict_order: fs_dist_cg / cg2 / gram_diag / pcg (both schemes) / pcgn are the models' and the single-device
   solvers' on A and the caller's A'; scheme 1 slices by the caller's cuts; default mode within test_gpu_dist_pcg.py's bars.
4  what the handle reports, what it refuses, a released shard of A' reached through At.
5  A, At and the pair walked together: products and option flips, every result exact, every guard intact.
6  two host threads on two handles that share a side.
7  all six orders of destroying the three; device memory comes back."""
import ctypes as C
import itertools
import threading

import numpy as np
import pytest

import _cg_model as M
import _dist_pair as DPair
import _dist_solvers as DV
import _exact as E
import _gpu as G
import _lifecycle as LC
import _pcg_model as P
import _pcgn_model as N
import _solvers as SV
from _gpu import FS_ERR_RELEASED, FS_OK, L  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-12                                              # the project's bar for a product in the default mode, row-scaled
# fs_dist_pcg runs on the recipes and on the named systems whose model is quick
PCG_SET = DPair.RECIPES0 + ("binary_F65", "cap_tol0", "lambda0_empty_column", "valued", "zero_rhs", "three_eigenvalues")
EXACT_SETS = ("wide_range", "subnormal", "subnormal_pattern", "zeros")
KS = (2, 4, 5)
_SINGLE = {}


# ---- 0 ---------------------------------------------------------------------------------------------------------------------
def _fits(s, route, ranks):
    """(three unknowns have no room for five ranks' cuts [2, 0, F - 5, 0, 3])"""
    return not (route == "cuts" and ranks == 5 and s.ncol < 5)


class _Exact:
    """an exact set of tests/_exact.py (row-major COO) with a System's surface, for PairDist"""

    def __init__(self, d):
        self.d, self.r = d, LC.refs_of(d)
        self.name, self.nrow, self.ncol, self.rows, self.cols, self.vals = d.name, d.nrow, d.ncol, d.rows, d.cols, d.vals

    def a_csr(self):
        return self.r.csr[0]

    def t_csr_coo(self):
        return self.r.csr[1]                                 # (rows ascend in the COO: the caller's order is the sorted one)


def _exact(name):
    if name not in _SINGLE:
        _SINGLE[name] = _Exact(LC.data_sets()[name])
    return _SINGLE[name]


@pytest.mark.parametrize("ranks", [1, 3, 5])
@pytest.mark.parametrize("route", DPair.ROUTES)
def test_the_shards_are_the_callers_arrays(L, route, ranks):
    for name, s in DV.PAIR_SYSTEMS.items():
        if not _fits(s, route, ranks):
            continue
        pd = DV.PairDist(L, s, ranks, route)
        try:
            bounds = pd.bounds_t()
            assert bounds[0] == 0 and bounds[-1] == s.ncol
            pd.t_csr()
            if route == "dev" and ranks >= 3:
                assert pd.bounds_of(pd.A)[:4] == [0, s.nrow // 2, s.nrow // 2, s.nrow]
            assert pd.bounds_of(pd.M) == pd.bounds_of(pd.A)
        finally:
            pd.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def _nan(shape, hbm):
    return G.put(np.full(shape, np.nan), hbm)


def _call(L, f, *a):
    from libfastsparse_amd import capi
    rc = f(*[capi._ptr(v) if hasattr(v, "shape") else v for v in a])
    assert rc == FS_OK, (f.__name__, rc, L.fs_last_error())


def _products(L, h, csr, t_csr, nrow, ncol, x, u, X, U, lam, hbm, same):
    """every transposed entry point of the pair h, and the direct ones, on the given inputs: {name: (got, want)} with `want` the
    oracle's storage-order products; outputs prefilled with NaN, inputs unchanged"""
    from oracle import pyoracle as O
    (arp, acc, avv), (trp, tcc, tvv) = csr, t_csr
    out = {}
    xi, ui = G.put(x, hbm), G.put(u, hbm)
    z = _nan(ncol, hbm)
    _call(L, L.fs_dist_spmv_t, h, z, ui)
    out["spmv_t"] = (G.to_numpy(z), O.csr_mul(ncol, trp, tcc, tvv, u))
    y = _nan(nrow, hbm)
    _call(L, L.fs_dist_spmv, h, y, xi)
    yw = O.csr_mul(nrow, arp, acc, avv, x)
    out["spmv"] = (G.to_numpy(y), yw)
    for l in (0.0, lam):
        z = _nan(ncol, hbm)
        _call(L, L.fs_dist_ata, h, z, xi, C.c_double(l))
        w = O.csr_mul(ncol, trp, tcc, tvv, yw)
        out[f"ata lambda {l}"] = (G.to_numpy(z), w + np.float64(l) * x if l != 0.0 else w)        # (fs_axpy: z += lambda x, two roundings)
    for k, Xk in X.items():
        Uk = U[k]
        Xi, Ui = G.put(Xk, hbm), G.put(Uk, hbm)
        Z = _nan((ncol, k), hbm)
        _call(L, L.fs_dist_spmm_t, h, Z, Ui, k)
        out[f"spmm_t k {k}"] = (G.to_numpy(Z), O.csr_mul_n(ncol, trp, tcc, tvv, Uk, k))
        Y = _nan((nrow, k), hbm)
        _call(L, L.fs_dist_spmm, h, Y, Xi, k)
        out[f"spmm k {k}"] = (G.to_numpy(Y), O.csr_mul_n(nrow, arp, acc, avv, Xk, k))
        assert same(G.to_numpy(Xi), Xk) and same(G.to_numpy(Ui), Uk), (k, "an input changed")
    assert same(G.to_numpy(xi), x) and same(G.to_numpy(ui), u), "an input changed"
    assert all(g.shape == w.shape for g, w in out.values())
    return out


def _resident(L, pd, nrow, ncol, x):
    """fs_dist_spmv_t_resident after fs_dist_spmv_resident: x once on every rank, y and z complete on every rank"""
    for r in range(pd.ranks):
        assert L.fs_copy_to_device(L.fs_dist_x(pd.M, r), x.ctypes.data, 8 * ncol) == 0
    assert L.fs_dist_spmv_resident(pd.M) == 0, L.fs_last_error()
    assert L.fs_dist_spmv_t_resident(pd.M) == 0, L.fs_last_error()
    got = []
    for r in range(pd.ranks):
        y, z = np.full(nrow, np.nan), np.full(ncol, np.nan)
        assert L.fs_copy_to_host(y.ctypes.data, L.fs_dist_y(pd.M, r), 8 * nrow) == 0
        assert L.fs_copy_to_host(z.ctypes.data, L.fs_dist_z(pd.M, r), 8 * ncol) == 0
        got.append((y, z))
    return got


def _direct_is_As(L, pd, x, X):
    """the direct side through the pair is the same call through A, bit for bit"""
    s = pd.s
    ys = []
    for h in (pd.M, pd.A):
        y = np.full(s.nrow, np.nan)
        _call(L, L.fs_dist_spmv, h, y, x)
        ys.append([y])
        for k, Xk in X.items():
            Y = np.full((s.nrow, k), np.nan)
            _call(L, L.fs_dist_spmm, h, Y, Xk, k)
            ys[-1].append(Y)
    for a, b in zip(*ys):
        assert E.bits_equal(a, b) and not np.isnan(a).any(), (s.name, a.shape, E.first_mismatch(a, b))


@pytest.mark.parametrize("ranks", [3, 5])
@pytest.mark.parametrize("route", DPair.ROUTES)
def test_products_strict_add_in_the_callers_order(L, route, ranks):
    from oracle import pyoracle as O
    for name in DPair.NAMED:
        s = DV.PAIR_SYSTEMS[name]
        if not _fits(s, route, ranks):
            continue
        rng = np.random.default_rng([2, ranks, s.ncol])
        x, u = rng.standard_normal(s.ncol), rng.standard_normal(s.nrow)
        X, U = {k: rng.standard_normal((s.ncol, k)) for k in KS}, {k: rng.standard_normal((s.nrow, k)) for k in KS}
        pd = DV.PairDist(L, s, ranks, route)
        try:
            t = pd.t_csr()
            with G.options(strict_order=1):
                for hbm in (False, True):
                    for what, (got, want) in _products(L, pd.M, pd.csr, t, s.nrow, s.ncol, x, u, X, U, 0.75, hbm, E.bits_equal).items():
                        assert E.bits_equal(got, want), (name, route, ranks, hbm, what, E.first_mismatch(got, want))
                yw = O.csr_mul(s.nrow, *pd.csr, x)
                zw = O.csr_mul(s.ncol, *t, yw)
                for r, (y, z) in enumerate(_resident(L, pd, s.nrow, s.ncol, x)):
                    assert E.bits_equal(y, yw) and E.bits_equal(z, zw), (name, route, ranks, "resident", r, E.first_mismatch(z, zw))
                _direct_is_As(L, pd, x, X)
        finally:
            pd.close()


@pytest.mark.parametrize("name", EXACT_SETS)
@pytest.mark.parametrize("mode", [m for m in G.SOLVER_MODES if m != "strict_order"])
def test_products_are_exact_on_the_exact_sets(L, mode, name):
    s = _exact(name)
    d, r = s.d, s.r
    lam = 2.0
    try:
        ata_lam = [E.ata(d.nrow, d.ncol, d.rows, d.cols, d.vals, r.inp[0][:, j], lam) for j in range(len(r.ata))]
    except AssertionError:                                   # (A'A x + lam x is exact only on some sets: exact_sum says on which)
        ata_lam = []
    for route, ranks in itertools.product(DPair.ROUTES, (3, 5)):
        pd = DV.PairDist(L, s, ranks, route)
        try:
            pd.bounds_t()
            pd.t_csr()
            with G.mode_options(mode):
                for hbm in (False, True):
                    j = 1 + int(hbm) + ranks
                    calls = [(L.fs_dist_spmv_t, 1, 1), (L.fs_dist_spmv, 0, 1)] + [(f, side, k) for k in KS for f, side in
                                                                              ((L.fs_dist_spmm_t, 1), (L.fs_dist_spmm, 0))]
                    for f, side, k in calls:
                        xin, want = r.run("in", side, j, k), r.run("out", side, j, k)
                        vi, vo = G.put(xin, hbm), _nan(want.size, hbm)
                        _call(L, f, pd.M, vo, vi, *([k] if k > 1 else []))
                        what = (name, mode, route, ranks, hbm, f.__name__, k)
                        assert E.bits_equal(G.to_numpy(vo), want), (what, E.first_mismatch(G.to_numpy(vo), want))
                        assert E.bits_equal(G.to_numpy(vi), xin), (what, "the input changed")
                    for jj, want in enumerate(r.ata):
                        for l, w in [(0.0, want)] + ([(lam, ata_lam[jj])] if ata_lam else []):
                            xin = r.run("in", 0, jj, 1)
                            vi, vo = G.put(xin, hbm), _nan(w.size, hbm)
                            _call(L, L.fs_dist_ata, pd.M, vo, vi, C.c_double(l))
                            assert E.bits_equal(G.to_numpy(vo), w), (name, mode, route, ranks, hbm, "ata", l, E.first_mismatch(G.to_numpy(vo), w))
                            assert E.bits_equal(G.to_numpy(vi), xin)
                if r.ata:
                    x = r.run("in", 0, 0, 1)
                    for rank, (y, z) in enumerate(_resident(L, pd, d.nrow, d.ncol, x)):
                        assert E.bits_equal(y, r.run("out", 0, 0, 1)) and E.bits_equal(z, r.ata[0]), (name, mode, route, ranks, "resident", rank)
        finally:
            pd.close()


@pytest.mark.parametrize("ranks", [3, 5])
@pytest.mark.parametrize("route", DPair.ROUTES)
def test_products_on_arbitrary_data_default_mode(L, route, ranks):
    """`valued` in the default mode: |got - want| <= 1e-12 sum |a| |x| row by row, `want` the oracle's product on the caller's A'.  A'(A x):
    the product A' y' of the device's own y' = y + e, |e| <= 1e-12 |A| |x|, is within 1e-12 |A'| |y'| of A' y', and A' y' within
    |A'| |e| of A' y: both are at most 1e-12 |A'| (|A| |x|) up to second order, so the bar is twice that, plus one rounding of
    z + lambda x"""
    from oracle import pyoracle as O
    s = DV.PAIR_SYSTEMS["valued"]
    rng = np.random.default_rng([3, ranks])
    x, u = rng.standard_normal(s.ncol), rng.standard_normal(s.nrow)
    X, U = {k: rng.standard_normal((s.ncol, k)) for k in KS}, {k: rng.standard_normal((s.nrow, k)) for k in KS}
    pd = DV.PairDist(L, s, ranks, route)
    try:
        t = pd.t_csr()
        (arp, acc, avv), (trp, tcc, tvv) = pd.csr, t
        scale_a = lambda v: O.csr_abs_scale(s.nrow, arp, acc, avv, v)
        scale_t = lambda v: O.csr_abs_scale(s.ncol, trp, tcc, tvv, v)
        per_column = lambda f, V: np.stack([f(np.ascontiguousarray(V[:, j])) for j in range(V.shape[1])], 1)
        two = 2.0 * scale_t(scale_a(x))
        bars = {"spmv_t": scale_t(u), "spmv": scale_a(x), "ata lambda 0.0": two, "ata lambda 0.75": two + 2.0 * np.abs(0.75 * x)}
        for k in KS:
            bars[f"spmm_t k {k}"], bars[f"spmm k {k}"] = per_column(scale_t, U[k]), per_column(scale_a, X[k])
        for hbm in (False, True):
            got = _products(L, pd.M, pd.csr, t, s.nrow, s.ncol, x, u, X, U, 0.75, hbm, E.bits_equal)
            assert set(got) == set(bars)
            for what, (g, w) in got.items():
                err = np.abs(g - w) / np.maximum(bars[what], 1e-300)
                print(f"{route} {ranks} ranks {'HBM' if hbm else 'host'} {what}: worst error {err.max():.3g} of the row scale")
                assert np.all(np.abs(g - w) <= TOL * np.maximum(bars[what], 1e-300)), (route, ranks, hbm, what, float(err.max()))
        _direct_is_As(L, pd, x, X)
    finally:
        pd.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def _single_handles(L, s):
    """A from its CSR and the caller's A' from its own, as the pair's shards hold them, on one device"""
    from libfastsparse_amd import capi
    if s.name not in _SINGLE:
        (arp, acc, avv), (trp, tcc, tvv) = s.a_csr(), s.t_csr_coo()
        A = capi.Matrix.from_csr(s.nrow, s.ncol, G.to_device(arp), G.to_device(acc), None if avv is None else G.to_device(avv))
        At = capi.Matrix.from_csr(s.ncol, s.nrow, G.to_device(trp), G.to_device(tcc), None if tvv is None else G.to_device(tvv))
        _SINGLE[s.name] = (A, At)
    return _SINGLE[s.name]


def _model_bounds(pd):
    """the slices of the scheme-1 models: the cuts the pair reports for A' (which are At's, and what the caller chose)"""
    return pd.bounds_t()


def _fs_cg2_on(L, A, At, s):
    from libfastsparse_amd import capi
    x, it = G.nan_vector(2 * s.ncol), C.c_int(-1)
    capi.check(L.fs_cg2(A.h, At.h, x.data_ptr(), G.to_device(s.B.reshape(-1)).data_ptr(), s.lam, s.tol, C.byref(it), capi.current_stream()), "fs_cg2")
    return x.cpu().numpy().reshape(-1, 2), it.value, SV.cg_state(L, True)


@pytest.mark.parametrize("route,ranks", [("coo", 3), ("cuts", 3), ("dev", 3), ("cuts", 5), ("coo", 1)])
def test_cg_scheme0_strict_is_the_model_and_fs_cg(L, route, ranks):
    for name in DPair.NAMED:
        s = DV.PAIR_SYSTEMS[name]
        if not _fits(s, route, ranks):
            continue
        pd = DV.PairDist(L, s, ranks, route)
        try:
            pd.t_csr()
            with G.options(strict_order=1, dist_cg_scheme=0):
                for two in ((False, True) if s.two else (False,)):
                    x, it, st = pd.cg(two)
                    entry = f"fs_dist_cg{'2' if two else ''} scheme 0 on a pair, route {route}, {ranks} ranks"
                    SV.assert_cg_model(entry, s, two, x, it, st, SV.cg_model(s, two, "coo"))
                    if route == "coo" and ranks == 3:
                        A, At = _single_handles(L, s)
                        xs, its, sts = _fs_cg2_on(L, A, At, s) if two else SV.fs_cg_on(L, A, At, s)
                        bad = M.mismatch(x, xs, it, its, st, sts)
                        assert bad is None, f"{entry} vs fs_cg{'2' if two else ''} on {name}: {bad}"
        finally:
            pd.close()


@pytest.mark.parametrize("route,ranks", [("coo", 3), ("cuts", 3), ("cuts", 5)])
def test_cg_scheme1_strict_slices_by_the_pairs_cuts(L, route, ranks):
    """the slice model on pair.bounds_t(): with the caller's cuts an empty slice in front and a one-row slice (three ranks), empty
    slices in the middle (five)"""
    for name in DPair.NAMED:
        s = DV.PAIR_SYSTEMS[name]
        if not _fits(s, route, ranks):
            continue
        pd = DV.PairDist(L, s, ranks, route)
        try:
            bounds = _model_bounds(pd)
            pd.t_csr()
            with G.options(strict_order=1, dist_cg_scheme=1):
                x, it, st = pd.cg(False)
            SV.assert_cg_model(f"fs_dist_cg scheme 1 on a pair, route {route}, bounds {bounds}", s, False, x, it, st, SV.cg_model(s, False, "coo", bounds))
        finally:
            pd.close()


def _single_gram_diag(L, s, lam):
    from libfastsparse_amd import capi
    key = ("gram", s.name, lam)
    if key not in _SINGLE:
        one = G.nan_vector(s.ncol)
        capi.gram_diag(_single_handles(L, s)[1], lam, one, capi.current_stream())
        _SINGLE[key] = one.cpu().numpy()
    return _SINGLE[key]


@pytest.mark.parametrize("ranks", [1, 3, 5])
@pytest.mark.parametrize("route", DPair.ROUTES)
def test_gram_diag_is_fs_gram_diag_on_the_callers_at(L, route, ranks):
    from libfastsparse_amd import capi
    for name, s in DV.PAIR_SYSTEMS.items():
        if not _fits(s, route, ranks):
            continue
        pd = DV.PairDist(L, s, ranks, route)
        try:
            t = pd.t_csr()
            for lam in (s.lam, 0.0, 0.75):
                want = _single_gram_diag(L, s, lam)
                assert M.same_bits(want, P.gram_diag(t, lam)).all(), (name, lam, "fs_gram_diag is not its model")
                for hbm in (False, True):
                    d = _nan(s.ncol, hbm)
                    capi.dist_gram_diag(pd.M, lam, d)
                    ok = M.same_bits(G.to_numpy(d), want)
                    assert ok.all(), (name, route, ranks, lam, hbm, int((~ok).sum()), int(np.flatnonzero(~ok)[0]))
                if lam == 0.0 and name == "lambda0_empty_column":
                    assert np.diff(t[0])[5] == 0 and G.to_numpy(d)[5] == 0.0 and not np.signbit(G.to_numpy(d)[5])
        finally:
            pd.close()


@pytest.mark.parametrize("name", PCG_SET)
def test_pcg_scheme0_strict_is_fs_pcg_on_the_callers_at(L, name):
    s = DV.PAIR_SYSTEMS[name]
    for route, ranks in (("coo", 3), ("cuts", 5), ("dev", 3), ("cuts", 1)):
        if not _fits(s, route, ranks):
            continue
        pd = DV.PairDist(L, s, ranks, route)
        try:
            t = pd.t_csr()
            with G.options(strict_order=1, dist_cg_scheme=0):
                for case in range(len(SV.CASES)):
                    what, precond, x0, max_iter, diag = DV.case_args(s, case, t)
                    hbm = (case + ranks) % 2 == 1
                    x, info, st = DV.dpcg(L, pd, s, precond, x0, max_iter, diag, hbm=hbm)
                    model = DV.dpcg_model(s, case, t)
                    entry = f"fs_dist_pcg scheme 0 on a pair, {what}, route {route}, {ranks} ranks, {'HBM' if hbm else 'host'} vectors"
                    bad = M.mismatch(x, model.x, info.iterations, model.iterations, st, model.state)
                    assert bad is None, f"{entry} on {name}: {bad}"
                    SV.assert_info((name, entry), info, model)
                    if route == "coo":
                        A, At = _single_handles(L, s)
                        xs, infos, _ = SV.pcg_run(L, A, At, s, precond, x0, max_iter, diag)
                        assert M.same_bits(x, xs).all() and (info.iterations, info.converged) == (infos.iterations, infos.converged), entry
                        assert M.same_bits(info.rnorm, infos.rnorm)[0] and M.same_bits(info.bnorm, infos.bnorm)[0], entry
        finally:
            pd.close()


@pytest.mark.parametrize("name,route,ranks", [(n, ro, ra) for n in PCG_SET for ro, ra in (("coo", 3), ("cuts", 3), ("cuts", 5))
                                              if _fits(DV.PAIR_SYSTEMS[n], ro, ra)])
def test_pcg_scheme1_strict_slices_by_the_pairs_cuts(L, name, route, ranks):
    s = DV.PAIR_SYSTEMS[name]
    pd = DV.PairDist(L, s, ranks, route)
    try:
        bounds = _model_bounds(pd)
        t = pd.t_csr()
        with G.options(strict_order=1, dist_cg_scheme=1):
            for case in range(len(SV.CASES)):
                what, precond, x0, max_iter, diag = DV.case_args(s, case, t)
                hbm = case % 2 == 1
                x, info, st = DV.dpcg(L, pd, s, precond, x0, max_iter, diag, hbm=hbm)
                model = DV.dpcg_model(s, case, t, bounds)
                bad = M.mismatch(x, model.x, info.iterations, model.iterations, st, model.state)
                assert bad is None, f"fs_dist_pcg scheme 1 on a pair, {what}, route {route}, bounds {bounds}, on {name}: {bad}"
                SV.assert_info((name, what, bounds), info, model)
    finally:
        pd.close()


@pytest.mark.parametrize("k", DV.KS)
def test_pcgn_columns_are_fs_pcgn_and_the_model(L, k):
    s, B = DV.panel(k)
    case = k % len(SV.CASES)
    single = _single_handles(L, s)
    for route, ranks in (("coo", 3), ("cuts", 5)):
        pd = DV.PairDist(L, s, ranks, route)
        try:
            t = pd.t_csr()
            what, precond, x0, max_iter, diag = DV.case_args(s, case, t)
            X0 = SV.x0_columns(s, B) if x0 is not None else None
            key = ("pcgn on the caller's A'", k, case)
            if key not in _SINGLE:
                am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t)
                dinv = None if precond == P.PRECOND_NONE else P.dinv_of(P.gram_diag(t, s.lam) if precond == P.PRECOND_JACOBI else diag)
                _SINGLE[key] = N.pcgn(s.ncol, am, atm, B, s.lam, s.tol, max_iter, dinv, X0)
            model = _SINGLE[key]
            with G.options(strict_order=1):
                X, infos, st, cs = DV.dpcgn(L, pd, s, B, precond, X0, max_iter, diag, hbm=ranks == 3)
                Xs, infos_s, _, cs_s = SV.pcgn_run(L, single[0], single[1], s, B, precond, X0, max_iter, diag)
                with G.options(dist_cg_scheme=1):                  # replicated whatever the scheme says
                    X1, infos1, _, _ = DV.dpcgn(L, pd, s, B, precond, X0, max_iter, diag)
                if k == 1:                                       # one column is fs_dist_pcg
                    with G.options(dist_cg_scheme=0):
                        x, info, _ = DV.dpcg(L, pd, s, precond, None if X0 is None else X0[:, 0], max_iter, diag, b=B[:, 0])
                    assert M.same_bits(X[:, 0], x).all() and (infos[0].iterations, infos[0].converged) == (info.iterations, info.converged)
                    assert M.same_bits(infos[0].rnorm, info.rnorm)[0] and M.same_bits(infos[0].bnorm, info.bnorm)[0]
            assert len(infos) == k
            assert M.same_bits(X1, X).all() and [i.iterations for i in infos1] == [i.iterations for i in infos], (k, route)
            for j in range(k):
                SV.assert_column((k, route, ranks, what, j, "model"), X[:, j], infos[j], cs[j], model.X[:, j], model.infos[j], model.columns[j].state)
                SV.assert_column((k, route, ranks, what, j, "fs_pcgn"), X[:, j], infos[j], cs[j], Xs[:, j], N.Info(infos_s[j].iterations,
                                  infos_s[j].converged, infos_s[j].rnorm, infos_s[j].bnorm))
                assert all(M.same_bits(cs[j][f], cs_s[j][f])[0] for f in N.PN), (k, route, j, cs[j], cs_s[j])
            assert st["iter"] == max(i.iterations for i in infos), (k, route, st)
        finally:
            pd.close()


@pytest.mark.parametrize("route", ["coo", "cuts"])
def test_default_mode_within_the_bars_of_built_transposes(L, route):
    """Jacobi and no preconditioner on the column-scaled recipe, both schemes: test_gpu_dist_pcg.py's bars, by the function they share.  A
    caller's diagonal that is Jacobi's own d gives Jacobi's bits (the bar of test_released_shard_of_the_transpose there)"""
    from libfastsparse_amd import capi
    s = DV.PAIR_SYSTEMS["scaled_seed0"]
    pd = DV.PairDist(L, s, 3, route)
    try:
        pd.t_csr()
        DV.assert_default_mode_bars(L, pd, s)
        kept = np.full(s.ncol, np.nan)
        capi.dist_gram_diag(pd.M, s.lam, kept)
        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                xj, ij, _ = DV.dpcg(L, pd, s, P.PRECOND_JACOBI)
                xd, idg, _ = DV.dpcg(L, pd, s, P.PRECOND_DIAG, diag=kept)
            assert idg.converged == 1 and idg.iterations == ij.iterations and M.same_bits(xd, xj).all(), (route, scheme)
    finally:
        pd.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_what_the_handle_reports(L):
    s = DV.PAIR_SYSTEMS["binary_F65"]
    for route in DPair.ROUTES:
        pd = DV.PairDist(L, s, 3, route)
        try:
            assert L.fs_dist_matrix_has_transpose(pd.M) == 1 and L.fs_dist_matrix_has_transpose(pd.A) == 0
            assert L.fs_dist_matrix_nnz(pd.M) == L.fs_dist_matrix_nnz(pd.A) == s.rows.size
            for r in range(3):
                assert L.fs_dist_matrix_shard(pd.M, r, 0) == L.fs_dist_matrix_shard(pd.A, r, 0) != None   # noqa: E711
                assert L.fs_dist_matrix_shard(pd.M, r, 1) == L.fs_dist_matrix_shard(pd.At, r, 0) != None  # noqa: E711
                assert L.fs_dist_matrix_shard_nnz(pd.M, r) == L.fs_dist_matrix_shard_nnz(pd.A, r)
            # a transpose is there: both builders say FS_OK and build nothing -- the shared side keeps the caller's arrays
            t = pd.t_csr()
            u = np.random.default_rng(4).standard_normal(s.nrow)
            z0 = np.full(s.ncol, np.nan)
            _call(L, L.fs_dist_spmv, pd.At, z0, u)
            rp, cc, vv = pd.csr
            assert L.fs_dist_matrix_build_transpose(pd.M, rp.ctypes.data, cc.ctypes.data, None) == FS_OK, L.fs_last_error()
            assert L.fs_dist_matrix_build_transpose_device(pd.M) == FS_OK, L.fs_last_error()
            assert DPair.same_arrays(pd.t_csr(), t) and L.fs_dist_matrix_has_transpose(pd.At) == 0
            z1 = np.full(s.ncol, np.nan)
            _call(L, L.fs_dist_spmv, pd.At, z1, u)
            assert E.bits_equal(z0, z1) and not np.isnan(z1).any()
        finally:
            pd.close()


def test_refusals_leak_nothing(L):
    import torch
    s = DV.PAIR_SYSTEMS["binary_F65"]
    pd, other = DV.PairDist(L, s, 3, "coo"), DV.PairDist(L, s, 3, "coo")
    try:
        ok = L.fs_dist_matrix_pair(pd.A, pd.At)              # (warm-up: whatever the process keeps for good exists now)
        assert ok
        L.fs_dist_matrix_destroy(ok)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        refused = {"NULL A": (None, pd.At), "NULL At": (pd.A, None), "two contexts": (pd.A, other.At), "two contexts, the other way": (other.A, pd.At),
                   "A with A": (pd.A, pd.A), "At with At": (pd.At, pd.At), "a pair's shape with A": (pd.M, pd.A)}
        for _ in range(20):
            for what, (a, at) in refused.items():
                assert not L.fs_dist_matrix_pair(a, at), what
                assert L.fs_last_error().startswith(b"fs_dist_matrix_pair:"), (what, L.fs_last_error())
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        assert free1 >= free0, (free0, free1, "a refused fs_dist_matrix_pair kept device memory")
        x, it, _ = pd.cg(False)                              # and the handles still work
        assert np.isfinite(x).all()
    finally:
        pd.close()
        other.close()


def test_released_shard_of_the_transpose_reached_through_at(L):
    """fs_matrix_release_csr on ONE rank's shard of the shared side, through At: the pair's Jacobi is refused before anything is
    written; a diagonal kept from before still solves, with the same bits"""
    from libfastsparse_amd import capi
    s = DV.PAIR_SYSTEMS["scaled_seed0"]
    with G.options(binning=2, bin_flags=64):                           # kept two-pass copies: there is something to release for
        pd = DV.PairDist(L, s, 3, "coo")
    try:
        kept = np.full(s.ncol, np.nan)
        capi.dist_gram_diag(pd.M, s.lam, kept)
        B = SV.columns(s, 2)
        before = {}
        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                before[scheme] = DV.dpcg(L, pd, s, P.PRECOND_JACOBI)
                assert before[scheme][1].converged == 1
        X_before = DV.dpcgn(L, pd, s, B, P.PRECOND_JACOBI)[0]
        assert L.fs_matrix_release_csr(L.fs_dist_matrix_shard(pd.At, 1, 0)) == 1
        prm = capi.PcgParams(s.tol, 0, P.PRECOND_JACOBI, 0, None)
        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                x, X, d = np.full(s.ncol, np.nan), np.full(B.shape, np.nan), np.full(s.ncol, np.nan)
                bits, Bits = x.view(np.int64).copy(), X.view(np.int64).copy()
                assert L.fs_dist_pcg(pd.M, x.ctypes.data, s.b.ctypes.data, s.lam, C.byref(prm), None) == FS_ERR_RELEASED
                assert b"fs_matrix_release_csr" in L.fs_last_error()
                assert L.fs_dist_pcgn(pd.M, X.ctypes.data, B.ctypes.data, 2, s.lam, C.byref(prm), None) == FS_ERR_RELEASED
                assert L.fs_dist_gram_diag(pd.M, s.lam, d.ctypes.data) == FS_ERR_RELEASED
                assert np.array_equal(x.view(np.int64), bits) and np.array_equal(X.view(np.int64), Bits) and np.isnan(d).all()
                x_diag, info_diag, _ = DV.dpcg(L, pd, s, P.PRECOND_DIAG, diag=kept)   # Jacobi's own d, kept: the same dinv, the same bits
                assert info_diag.converged == 1 and info_diag.iterations == before[scheme][1].iterations, scheme
                assert M.same_bits(x_diag, before[scheme][0]).all(), scheme
        assert M.same_bits(DV.dpcgn(L, pd, s, B, P.PRECOND_DIAG, diag=kept)[0], X_before).all()
    finally:
        pd.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
FLIPS = {"reproducible": (0, 1), "strict_order": (0, 1), "spmv_kernel": (0, 1, 7), "spmm_kernel": (0, 1, 3), "cg_fixed_order": (1, 0)}
# the forced opening: (handle, operation, k) or a flip -- every step crosses state that two handles share
OPENING = [("P", "spmv", 1), ("flip", "strict_order", 0), ("A", "spmv", 1), ("P", "spmv", 1), ("P", "spmm", 4), ("A", "spmm", 2),
           ("P", "spmm", 4), ("At", "spmm", 4), ("P", "spmm_t", 4)]


@pytest.mark.parametrize("name", ["wide_range", "subnormal_pattern", "wide_range_mid"])
def test_three_handles_that_share_shards_walked_together(L, name):
    """A, At and P = pair(A, At) on three virtual ranks: products on every side a handle has and option flips, in a seeded random
    order behind an opening that crosses the shared state on purpose -- a side's k = 1 plan made through one handle and used
    through another, k-column copies prepared on shards that another handle's k-column plan was made against.  Vectors in guarded
    HBM arenas and guarded host arrays; after every operation exact bits (tests/_exact.py), the input unchanged, all guards intact.
    The mid-size set with panels of 32 rows is created under strict_order, so the first default product has to plan again, and
    its products are really cut (asserted)"""
    from libfastsparse_amd import capi
    big = name == "wide_range_mid"
    if big:
        d = LC.mid_size()
        r = LC.refs_of(d, nc=2, ata_cols=0)
    else:
        d = LC.data_sets()[name]
        r = LC.refs_of(d)
    ks = (2,) if big else KS
    vals = None if d.vals is None else d.vals.ctypes.data
    rng = np.random.default_rng(78)
    mem = {"hbm": LC.TorchMem(), "host": LC.NumpyMem()}
    D = L.fs_dist_create(3, (C.c_int * 3)(0, 0, 0))
    assert D, L.fs_last_error()
    H = {}
    log = []
    try:
        with G.options(binning=2, bin_rows=32 if big else 256, strict_order=int(big)):
            H["A"] = L.fs_dist_csr_create(D, d.nrow, d.ncol, d.nnz, d.rp.ctypes.data, d.cols.ctypes.data, vals)
            assert H["A"], L.fs_last_error()
            H["At"] = L.fs_dist_coo_create(D, d.ncol, d.nrow, d.nnz, d.cols.ctypes.data, d.rows.ctypes.data, vals)
            assert H["At"], L.fs_last_error()
            H["P"] = capi.dist_matrix_pair(H["A"], H["At"])
        n = max(d.nrow, d.ncol)
        vec = {(where, role): LC.Guarded(mem[where], f"{role} vector in {where}", n * max(ks)) for where in ("hbm", "host") for role in ("in", "out")}
        # what a handle can do: (operation, side of the references, entry point's transposed flag)
        can = {"A": ("spmv", "spmm"), "At": ("spmv", "spmm"), "P": ("spmv", "spmm", "spmv_t", "spmm_t", "ata")}
        with G.options(**{k: L.fs_get_option(k.encode()) for k in FLIPS}):
            capi.set_option("strict_order", 1)
            for step in range(20 if big else 60):
                forced = OPENING[step] if step < len(OPENING) else None
                if forced:
                    who, op, k = forced
                else:
                    who = ("A", "At", "P")[int(rng.integers(3))]
                    op = (can[who] + ("flip",))[int(rng.integers(len(can[who]) + 1))]
                    k = int(rng.choice(ks)) if op.startswith("spmm") else 1
                if who == "flip" or op == "flip" or (op == "ata" and not r.ata):
                    k_, vs = list(FLIPS.items())[int(rng.integers(len(FLIPS)))]
                    v = vs[int(rng.integers(len(vs)))]
                    if forced:
                        k_, v = forced[1:]
                    log.append(f"{step} {k_} = {v}")
                    capi.set_option(k_, v)
                    continue
                k = min(k, max(ks)) if k > 1 else 1
                transposed = op.endswith("_t")
                side = int(transposed) if who != "At" else 1         # At's direct side is A': inputs over the rows of A, outputs over its columns
                where = "host" if rng.integers(2) else "hbm"
                wi, wo = ("host", "hbm")[int(rng.integers(2))], where
                j = int(rng.integers(len(r.ata) if op == "ata" else r.nc - k + 1))
                gi, go = vec[(wi, "in")], vec[(wo, "out")]
                xin = r.run("in", 0 if op == "ata" else side, j, k)
                want = r.ata[j] if op == "ata" else r.run("out", side, j, k)
                gi.mem.put(gi.place(xin.size, int(rng.integers(2))), xin)
                go.mem.fill_bits(go.place(want.size, int(rng.integers(2))), LC.PREFILLS["nan"])
                log.append(f"{step} {who} {op} k {k} column {j} in {wi} out {wo}")
                pi, po = gi.mem.ptr(gi.view), go.mem.ptr(go.view)
                if op == "ata":
                    rc = L.fs_dist_ata(H[who], po, pi, 0.0)
                elif k == 1:
                    rc = (L.fs_dist_spmv_t if transposed else L.fs_dist_spmv)(H[who], po, pi)
                else:
                    rc = (L.fs_dist_spmm_t if transposed else L.fs_dist_spmm)(H[who], po, pi, k)
                assert rc == 0, (rc, L.fs_last_error(), log[-12:])
                got = go.mem.get(go.view)
                assert E.bits_equal(got, want), (name, E.first_mismatch(got, want), log[-12:])
                assert gi.mem.eq(gi.view, gi.mem.const(xin)), ("input modified", log[-12:])
                for g in vec.values():
                    assert g.guards_ok(), (g.first_broken(), log[-12:])
                if big and step == 3:                                # the first default-mode products: planned again, and really cut
                    assert L.fs_debug_dist_parts(H["P"], 0) > 1 and L.fs_debug_dist_parts(H["A"], 0) > 1, log[-12:]
        assert len(log) == (20 if big else 60)
    finally:
        for h in ("P", "A", "At"):
            if h in H:
                L.fs_dist_matrix_destroy(H[h])
        L.fs_dist_destroy(D)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_two_host_threads_on_handles_that_share_a_side(L):
    """one thread: fs_dist_spmv + fs_dist_spmv_t on P; the other: fs_dist_spmv on At, whose direct side IS P's transposed side (its
    k = 1 plan, buffers and events): each handle has its own lock, only the context's orders the products.  Integer inputs, each
    thread its own vectors; every result is the single-threaded one bit for bit (the shape of test_two_host_threads_share_matrices)"""
    from oracle import pyoracle as O
    s = LC.pair_system("exact").s
    pd = DV.PairDist(L, s, 3, "coo")
    errors = []
    try:
        t = pd.t_csr()
        rng = np.random.default_rng(6)
        x, u = rng.integers(-512, 513, s.ncol).astype(np.float64), rng.integers(-512, 513, s.nrow).astype(np.float64)
        yw, zw = O.csr_mul(s.nrow, *pd.csr, x), O.csr_mul(s.ncol, *t, u)

        def once_p(y, z):
            assert L.fs_dist_spmv(pd.M, y.ctypes.data, x.ctypes.data) == 0, L.fs_last_error()
            assert L.fs_dist_spmv_t(pd.M, z.ctypes.data, y.ctypes.data) == 0, L.fs_last_error()

        def once_at(z):
            assert L.fs_dist_spmv(pd.At, z.ctypes.data, u.ctypes.data) == 0, L.fs_last_error()

        y1, z1, z2 = np.full(s.nrow, np.nan), np.full(s.ncol, np.nan), np.full(s.ncol, np.nan)
        once_p(y1, z1)
        once_at(z2)
        assert E.bits_equal(y1, yw) and E.bits_equal(z1, O.csr_mul(s.ncol, *t, yw)) and E.bits_equal(z2, zw), "single-threaded"

        def on_p():
            try:
                y, z = np.full(s.nrow, np.nan), np.full(s.ncol, np.nan)
                for i in range(25):
                    y.fill(np.nan)
                    z.fill(np.nan)
                    once_p(y, z)
                    if not (E.bits_equal(y, y1) and E.bits_equal(z, z1)):
                        errors.append(f"P, round {i}: {E.first_mismatch(y, y1)}; {E.first_mismatch(z, z1)}")
                        return
            except BaseException as ex:
                errors.append(repr(ex))

        def on_at():
            try:
                z = np.full(s.ncol, np.nan)
                for i in range(25):
                    z.fill(np.nan)
                    once_at(z)
                    if not E.bits_equal(z, z2):
                        errors.append(f"At, round {i}: {E.first_mismatch(z, z2)}")
                        return
            except BaseException as ex:
                errors.append(repr(ex))

        ts = [threading.Thread(target=on_p), threading.Thread(target=on_at)]
        for th in ts:
            th.start()
        for th in ts:
            th.join()
        assert not errors, errors
    finally:
        pd.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_every_order_of_destroying_the_three(L):
    """A, At and P destroyed in all six orders: after each destroy every surviving handle multiplies on each side it has; P with both
    parents gone still multiplies both ways and solves (Jacobi; the exact family: x = b / c at iteration 0).  After the last destroy
    free device memory is back where it was before the three were created, within one solve's work space (the comparison and the
    allowance of test_solver_work_space_is_given_back and test_interleaved_solves_share_the_work_space_and_give_it_back)"""
    import torch
    from libfastsparse_amd import capi
    from oracle import pyoracle as O
    fam = M.exact_family(False)
    s = fam.s
    a_csr, t_csr = fam.a_csr(), fam.t_csr()
    rng = np.random.default_rng(7)
    x, u = rng.integers(-512, 513, s.ncol).astype(np.float64), rng.integers(-512, 513, s.nrow).astype(np.float64)
    yw, zw = O.csr_mul(s.nrow, *a_csr, x), O.csr_mul(s.ncol, *t_csr, u)
    D = L.fs_dist_create(3, (C.c_int * 3)(0, 0, 0))
    assert D, L.fs_last_error()

    def product(h, f, n_out, vin, want, what):
        out = np.full(n_out, np.nan)
        assert f(h, out.ctypes.data, vin.ctypes.data) == 0, (what, L.fs_last_error())
        assert E.bits_equal(out, want), (what, E.first_mismatch(out, want))

    def use(H, what):
        if "A" in H:
            product(H["A"], L.fs_dist_spmv, s.nrow, x, yw, (what, "A"))
        if "At" in H:
            product(H["At"], L.fs_dist_spmv, s.ncol, u, zw, (what, "At"))
        if "P" in H:
            product(H["P"], L.fs_dist_spmv, s.nrow, x, yw, (what, "P direct"))
            product(H["P"], L.fs_dist_spmv_t, s.ncol, u, zw, (what, "P transposed"))

    def cycle(order):
        rp, cc, _ = a_csr
        H = {"A": L.fs_dist_csr_create(D, s.nrow, s.ncol, len(cc), rp.ctypes.data, cc.ctypes.data, None)}
        H["At"] = L.fs_dist_coo_create(D, s.ncol, s.nrow, s.rows.size, s.cols.ctypes.data, s.rows.ctypes.data, None)
        assert H["A"] and H["At"], L.fs_last_error()
        H["P"] = capi.dist_matrix_pair(H["A"], H["At"])
        try:
            use(H, (order, "all three"))
            for gone in order:
                L.fs_dist_matrix_destroy(H.pop(gone))
                use(H, (order, f"after {gone}"))
                if set(H) == {"P"}:
                    xs = np.full(s.ncol, np.nan)
                    info = capi.dist_pcg(H["P"], xs, s.b, s.lam, s.tol, precond=P.PRECOND_JACOBI)
                    assert info.converged == 1 and info.iterations == 0 and E.bits_equal(xs, s.b / fam.c), (order, info.iterations)
        finally:
            for h in H.values():
                L.fs_dist_matrix_destroy(h)

    try:
        orders = list(itertools.permutations(("A", "At", "P")))
        cycle(orders[3])                                     # (warm-up: whatever the process keeps for good exists now)
        one_solve = 8 * (3 * s.ncol + s.nrow + s.ncol + 2048 + 512)
        for order in orders:
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            cycle(order)
            torch.cuda.synchronize()
            free1 = torch.cuda.mem_get_info()[0]
            print(f"destroyed in the order {order}: free device memory {free0} bytes before the three, {free1} after; allowance {one_solve}")
            assert free0 - free1 <= one_solve, (order, free0, free1, one_solve)
    finally:
        L.fs_dist_destroy(D)
