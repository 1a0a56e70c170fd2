"""fs_dist_gram_diag, fs_dist_pcg and fs_dist_pcgn on virtual ranks of one device (fs_dist_create(n, [0] * n)), against the CPU models
(tests/_pcg_model.py, _dist_pcg_model.py, _pcgn_model.py) and against the single-device solvers, in the idioms of test_gpu_cg.py and
test_gpu_pcg.py.  A' of every model is dist.t_csr(): the shards' own rows, downloaded.

1  fs_dist_gram_diag has fs_gram_diag's bits on 1, 3 and 5 ranks, A' built on the host and on the device.
2  strict_order, scheme 0: fs_dist_pcg IS fs_pcg -- the model's x, info and st[], and a single-device fs_pcg on the same CSRs.
3  strict_order, scheme 1 on three ranks: the slice model (every rank reduces its slice, stage 2 adds the rank values); the recipes
   are first shown, on the CPU, to tell the two schemes apart; five ranks on three unknowns leave empty slices.
4  default mode on the column-scaled recipes: Jacobi converges within fs_pcg's bars, plain CG ends at the cap; solves repeat.
5  without a preconditioner, cold, uncapped: fs_dist_cg's x and count in every mode (b = 0: 0 and converged instead of NaN).
6  a solve that is done before its first iteration enqueues no product for an iteration.
7  fs_dist_pcgn: every column is fs_pcgn's on one device and the model's; k = 1 is fs_dist_pcg; "dist_cg_scheme" changes no bit.
8  statuses, with x / X untouched by every refused call.
9  guard zones, interleaved solves on one handle, device memory given back.
10 the number of sharded products per solve, for all four sharded solvers."""
import ctypes as C

import numpy as np
import pytest

import _cg_model as M
import _dist_pcg_model as DP
import _lifecycle as LC
import _pcg_model as P
import _pcgn_model as N
import test_gpu_cg as GC
import test_gpu_pcg as G
import test_gpu_pcgn as GN

pytestmark = pytest.mark.gpu

FS_OK, FS_ERR_ARG, FS_ERR_NO_TRANSPOSE, FS_ERR_RELEASED = 0, -2, -4, -5
CASES = G.CASES
RECIPES0 = {n: s for n, s in G.RECIPES.items() if n.endswith("seed0")}
ALL = dict({n: GC.SYSTEMS[n] for n in GC.DIST_SET}, **RECIPES0)
options = GC.options
_MODELS = {}


@pytest.fixture(scope="module")
def L():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from libfastsparse_amd import capi
    lib = capi.lib()
    lib.fs_debug_last_cg_state.argtypes = [C.c_void_p]
    lib.fs_debug_last_pcgn_state.argtypes = [C.c_void_p, C.c_int]
    lib.fs_debug_dist_products.restype = C.c_long
    lib.fs_debug_dist_products.argtypes = []
    lib.fs_debug_last_spmm_plan.argtypes = []
    return lib


def test_error_codes_are_the_header():
    import os
    with open(os.path.join(M.ROOT, "include", "fastsparse_hip.h")) as f:
        hdr = f.read()
    for name, v in (("FS_ERR_ARG", FS_ERR_ARG), ("FS_ERR_NO_TRANSPOSE", FS_ERR_NO_TRANSPOSE), ("FS_ERR_RELEASED", FS_ERR_RELEASED)):
        assert f"{name} = {v}" in " ".join(hdr.split()), name


def _put(a, hbm):
    """a vector where the caller keeps it: host memory, or HBM"""
    a = np.ascontiguousarray(a, np.float64)
    return G._d(a) if hbm else a.copy()


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else v


def dpcg(L, dist, s, precond=P.PRECOND_NONE, x0=None, max_iter=0, diag=None, tol=None, b=None, hbm=False):
    """fs_dist_pcg through capi.dist_pcg: x, fs_pcg_info, rank 0's final st[] by name"""
    from libfastsparse_amd import capi
    x = _put(np.full(s.ncol, np.nan) if x0 is None else x0, hbm)
    bd = _put(s.b if b is None else b, hbm)
    dd = None if diag is None else _put(diag, hbm)
    info = capi.dist_pcg(dist.M, x, bd, s.lam, s.tol if tol is None else tol, max_iter=max_iter, precond=precond, warm_start=x0 is not None,
                         diag=dd)
    return _np(x), info, P.state_from_device(G._raw_state(L))


def dpcgn(L, dist, s, B, precond=P.PRECOND_NONE, X0=None, max_iter=0, diag=None, tol=None, hbm=False):
    """fs_dist_pcgn through capi.dist_pcgn: X (F, k), the infos, st[] by name, rank 0's per-column scalars by name"""
    from libfastsparse_amd import capi
    k = B.shape[1]
    X = _put(np.full(B.shape, np.nan) if X0 is None else X0, hbm)
    infos = capi.dist_pcgn(dist.M, X, _put(B, hbm), s.lam, s.tol if tol is None else tol, max_iter=max_iter, precond=precond,
                           warm_start=X0 is not None, diag=None if diag is None else _put(diag, hbm))
    raw = np.full(N.MAX_RHS * N.PN_STRIDE, np.nan)
    assert L.fs_debug_last_pcgn_state(raw.ctypes.data, raw.size) == k * N.PN_STRIDE
    return _np(X), infos, P.state_from_device(G._raw_state(L)), N.state_from_device(raw, k)


def _case_args(s, case, t_csr):
    what, precond, warm, max_iter = CASES[case]
    diag = None
    if precond == P.PRECOND_DIAG:
        d = P.gram_diag(t_csr, s.lam)
        diag = np.abs(d) * (1.0 + 0.5 * np.cos(np.arange(s.ncol) * 1.7)) + 0.125
    return what, precond, (G._x0(s) if warm else None), max_iter, diag


def _model(s, case, t_csr, bounds=None):
    """the (slice) model of a case on the A' the shards hold; the sorted A' is the same for every rank count and either build (the
    entries of A' are part of the key: a pair handle holds the caller's order, tests/test_gpu_dist_pair.py)"""
    key = (s.name, case, None if bounds is None else tuple(bounds), t_csr[1].tobytes(), None if t_csr[2] is None else t_csr[2].tobytes())
    if key not in _MODELS:
        _, precond, x0, max_iter, diag = _case_args(s, case, t_csr)
        _MODELS[key] = DP.run(s, precond, max_iter=max_iter, x0=x0, t_csr=t_csr, diag=diag, bounds=bounds)
    return _MODELS[key]


def _sorted_t(dist, s):
    t_csr, want = dist.t_csr(), s.t_csr_sorted()
    assert all(np.array_equal(a, b) for a, b in zip(t_csr[:2], want[:2])), (s.name, "A' rows are not in ascending A-row order")
    return t_csr


def _single_handles(L, s):
    """A from its CSR and the sorted A', as the shards hold them, on one device"""
    from libfastsparse_amd import capi
    (arp, acc, avv), (trp, tcc, tvv) = s.a_csr(), s.t_csr_sorted()
    A = capi.Matrix.from_csr(s.nrow, s.ncol, G._d(arp), G._d(acc), None if avv is None else G._d(avv))
    At = capi.Matrix.from_csr(s.ncol, s.nrow, G._d(trp), G._d(tcc), None if tvv is None else G._d(tvv))
    return A, At


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_t", [False, True], ids=["host-transpose", "device-transpose"])
@pytest.mark.parametrize("ranks", [1, 3, 5])
def test_gram_diag_is_fs_gram_diag(L, ranks, device_t):
    from libfastsparse_amd import capi
    for name, s in ALL.items():
        dist = GC.Dist(L, s, ranks, device_t)
        try:
            t_csr = _sorted_t(dist, s)
            for lam in (s.lam, 0.0, 0.75):
                want = P.gram_diag(t_csr, lam)
                for hbm in (False, True):
                    d = _put(np.full(s.ncol, np.nan), hbm)
                    capi.dist_gram_diag(dist.M, lam, d)
                    ok = M.same_bits(_np(d), want)
                    assert ok.all(), (name, ranks, lam, hbm, int((~ok).sum()), int(np.flatnonzero(~ok)[0]))
                if lam == 0.0 and name == "lambda0_empty_column":
                    assert np.diff(t_csr[0])[5] == 0 and _np(d)[5] == 0.0 and not np.signbit(_np(d)[5])
            if ranks == 3 and not device_t:                          # fs_gram_diag on a single-device handle of the same CSR
                _, At = _single_handles(L, s)
                one = G._nan(s.ncol)
                capi.gram_diag(At, s.lam, one, capi.current_stream())
                assert M.same_bits(one.cpu().numpy(), P.gram_diag(t_csr, s.lam)).all(), name
        finally:
            dist.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALL))
def test_scheme0_strict_is_fs_pcg(L, name):
    s = ALL[name]
    single = {}
    for ranks, device_t in ((1, False), (3, False), (3, True), (1, True)):
        dist = GC.Dist(L, s, ranks, device_t)
        try:
            t_csr = _sorted_t(dist, s)
            with options(strict_order=1, dist_cg_scheme=0):
                for case in range(len(CASES)):
                    what, precond, x0, max_iter, diag = _case_args(s, case, t_csr)
                    hbm = (case + ranks) % 2 == 1
                    x, info, st = dpcg(L, dist, s, precond, x0, max_iter, diag, hbm=hbm)
                    model = _model(s, case, t_csr)
                    entry = f"fs_dist_pcg scheme 0 {what}, {ranks} ranks, {'device' if device_t else 'host'} A', {'HBM' if hbm else 'host'} vectors"
                    bad = M.mismatch(x, model.x, info.iterations, model.iterations, st, model.state)
                    assert bad is None, f"{entry} on {name}: {bad}"
                    G._assert_info((name, entry), info, model)
                    if ranks == 3 and not device_t:                  # a single-device fs_pcg on the same CSRs
                        if not single:
                            single["h"] = _single_handles(L, s)
                        xs, infos, _ = G.pcg_run(L, single["h"][0], single["h"][1], s, precond, x0, max_iter, diag)
                        assert M.same_bits(x, xs).all() and (info.iterations, info.converged) == (infos.iterations, infos.converged), entry
                        assert M.same_bits(info.rnorm, infos.rnorm)[0] and M.same_bits(info.bnorm, infos.bnorm)[0], entry
                    if name == "zero_rhs" and x0 is None:
                        assert info.converged == 1 and info.iterations == 0 and M.same_bits(x, np.zeros(s.ncol)).all()
        finally:
            dist.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALL))
def test_scheme1_strict_is_the_slice_model(L, name):
    s = ALL[name]
    for device_t in (False, True):
        dist = GC.Dist(L, s, 3, device_t)
        try:
            bounds = dist.bounds_t()
            assert bounds[0] == 0 and bounds[-1] == s.ncol
            t_csr = _sorted_t(dist, s)
            if name in RECIPES0:                                     # on the CPU first: the slice tree is told from the whole one
                whole, sliced = _model(s, 1, t_csr), _model(s, 1, t_csr, bounds)
                differ = int((~M.same_bits(whole.x, sliced.x)).sum())
                print(f"{name} bounds {bounds}: {differ} of {s.ncol} entries differ between the slice model and the whole model")
                assert all(a < b for a, b in zip(bounds, bounds[1:])) and differ >= 1, (name, bounds, differ)
            with options(strict_order=1, dist_cg_scheme=1):
                for case in range(len(CASES)):
                    what, precond, x0, max_iter, diag = _case_args(s, case, t_csr)
                    hbm = (case + int(device_t)) % 2 == 1
                    x, info, st = dpcg(L, dist, s, precond, x0, max_iter, diag, hbm=hbm)
                    model = _model(s, case, t_csr, bounds)
                    bad = M.mismatch(x, model.x, info.iterations, model.iterations, st, model.state)
                    assert bad is None, f"fs_dist_pcg scheme 1 {what}, bounds {bounds}, on {name}: {bad}"
                    G._assert_info((name, what, bounds), info, model)
        finally:
            dist.close()


def test_scheme1_with_empty_slices(L):
    """five ranks on the three rows of A': some slices are empty and contribute +0.0"""
    s = ALL["three_eigenvalues"]
    dist = GC.Dist(L, s, 5, False)
    try:
        bounds = dist.bounds_t()
        assert any(a == b for a, b in zip(bounds, bounds[1:])), bounds
        t_csr = _sorted_t(dist, s)
        with options(strict_order=1, dist_cg_scheme=1):
            for case in range(len(CASES)):
                what, precond, x0, max_iter, diag = _case_args(s, case, t_csr)
                x, info, st = dpcg(L, dist, s, precond, x0, max_iter, diag)
                model = _model(s, case, t_csr, bounds)
                bad = M.mismatch(x, model.x, info.iterations, model.iterations, st, model.state)
                assert bad is None, f"fs_dist_pcg scheme 1 {what}, bounds {bounds}: {bad}"
    finally:
        dist.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in G.RECIPES if n.startswith("scaled")])
def test_default_mode_jacobi_converges_where_plain_cg_does_not(L, name):
    s = G.RECIPES[name]
    dist = GC.Dist(L, s, 3, False)
    try:
        assert_default_mode_bars(L, dist, s)
    finally:
        dist.close()


def assert_default_mode_bars(L, dist, s):
    """the bars of a column-scaled recipe in the default mode, both schemes, on any handle with a transposed side (a built one here,
    a pair in test_gpu_dist_pair.py)"""
    name = s.name
    model = P.run(s, P.PRECOND_JACOBI)
    assert model.state["done"] == 1.0
    for scheme in (0, 1):
        with options(dist_cg_scheme=scheme):
            runs = [dpcg(L, dist, s, P.PRECOND_JACOBI) for _ in range(2)]
            plain = dpcg(L, dist, s)
        x, info, _ = runs[0]
        res = G._residual(s, x)
        print(f"{name} scheme {scheme}: jacobi {info.iterations} iterations (model {model.iterations}), true residual {res:.3g} "
              f"= {res / s.tol:.2f} tol; plain {plain[1].iterations} iterations, converged {plain[1].converged}")
        what = (name, scheme, info.iterations, model.iterations, res)
        assert info.converged == 1, what
        assert res <= 2 * s.tol, what
        assert abs(info.iterations - model.iterations) <= 1, what
        assert info.rnorm <= s.tol * info.bnorm, what
        assert runs[1][1].iterations == info.iterations and M.same_bits(runs[1][0], x).all(), what
        assert plain[1].converged == 0 and plain[1].iterations == s.ncol, (what, plain[1].iterations)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.MODES)
def test_without_preconditioner_cold_is_fs_dist_cg(L, mode):
    for name, s in ALL.items():
        dist = GC.Dist(L, s, 3, False)
        try:
            for scheme in (0, 1):
                with GC._mode(mode), options(dist_cg_scheme=scheme):
                    xc, itc, stc = dist.cg(False)
                    x, info, st = dpcg(L, dist, s)
                what = (name, mode, scheme)
                if name == "zero_rhs":
                    assert np.isnan(xc).all(), what
                    assert info.converged == 1 and info.iterations == 0 and M.same_bits(x, np.zeros(s.ncol)).all(), what
                    continue
                assert M.same_bits(x, xc).all() and info.iterations == itc, (what, M.mismatch(x, xc, info.iterations, itc))
                assert info.converged == int(stc["done"]), what
        finally:
            dist.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_no_product_for_a_finished_solve(L):
    """b = 0: no sharded product at all.  A warm start from the converged x of the solve before needs its residual, the one pair of
    products on x0 in front (scheme 1 takes the second half on the rank's own shard: one sharded product) -- and none for an iteration"""
    s = RECIPES0["scaled_seed0"]
    dist = GC.Dist(L, s, 3, False)
    try:
        for scheme, in_front in ((0, 2), (1, 1)):
            with options(dist_cg_scheme=scheme):
                before = L.fs_debug_dist_products()
                x, info, _ = dpcg(L, dist, s, P.PRECOND_JACOBI, b=np.zeros(s.ncol))
                assert L.fs_debug_dist_products() == before, scheme
                assert info.converged == 1 and info.iterations == 0 and info.bnorm == 0.0 and M.same_bits(x, np.zeros(s.ncol)).all()
                x1, info1, _ = dpcg(L, dist, s, P.PRECOND_JACOBI, tol=s.tol)
                assert info1.converged == 1 and info1.iterations > 0
                before = L.fs_debug_dist_products()
                x2, info2, _ = dpcg(L, dist, s, P.PRECOND_JACOBI, x0=x1, tol=s.tol * 10)
                assert L.fs_debug_dist_products() - before == in_front, (scheme, L.fs_debug_dist_products() - before)
                assert info2.converged == 1 and info2.iterations == 0 and M.same_bits(x2, x1).all(), scheme
        B = GN.columns(s, 3)
        before = L.fs_debug_dist_products()
        X, infos, _, _ = dpcgn(L, dist, s, np.zeros_like(B), P.PRECOND_JACOBI)
        assert L.fs_debug_dist_products() == before and all(i.converged == 1 and i.iterations == 0 for i in infos)
        assert M.same_bits(X, np.zeros_like(B)).all()
    finally:
        dist.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
KS = (1, 2, 3, 4, 5, 8, 17, 32)


def _panel(k):
    """the control recipe and k columns from _pcgn_model.recipe8's panel (a tiny and a huge column, a zero one, the top eigenvector:
    columns that freeze at different iterations), taken round and round with another scale each time"""
    s, B8, _ = N.recipe8("control")
    return s, np.ascontiguousarray(np.stack([B8[:, j % 8] * (1.0 + 0.25 * (j // 8)) for j in range(k)], 1))


@pytest.mark.parametrize("k", KS)
def test_pcgn_columns_are_fs_pcgn_and_the_model(L, k):
    s, B = _panel(k)
    case = k % len(CASES)
    single = _single_handles(L, s)
    for ranks in (1, 3):
        dist = GC.Dist(L, s, ranks, ranks == 3)
        try:
            t_csr = _sorted_t(dist, s)
            what, precond, x0, max_iter, diag = _case_args(s, case, t_csr)
            X0 = GN.x0_columns(s, B) if x0 is not None else None
            am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr)
            dinv = None if precond == P.PRECOND_NONE else P.dinv_of(P.gram_diag(t_csr, s.lam) if precond == P.PRECOND_JACOBI else diag)
            key = ("pcgn", k, case)
            if key not in _MODELS:
                _MODELS[key] = N.pcgn(s.ncol, am, atm, B, s.lam, s.tol, max_iter, dinv, X0)
            model = _MODELS[key]
            for kernel in ((1, 2) if k > 4 else (0,)):
                with options(strict_order=1, pcgn_kernel=kernel):
                    X, infos, st, cs = dpcgn(L, dist, s, B, precond, X0, max_iter, diag, hbm=ranks == 3)
                    Xs, infos_s, _, cs_s = GN.pcgn_run(L, single[0], single[1], s, B, precond, X0, max_iter, diag)
                    with options(dist_cg_scheme=1):                  # replicated whatever the scheme says
                        X1, infos1, _, _ = dpcgn(L, dist, s, B, precond, X0, max_iter, diag)
                assert len(infos) == k
                assert M.same_bits(X1, X).all() and [i.iterations for i in infos1] == [i.iterations for i in infos], (k, ranks, kernel)
                for j in range(k):
                    GN._assert_column((k, ranks, kernel, what, j, "model"), X[:, j], infos[j], cs[j], model.X[:, j], model.infos[j], model.columns[j].state)
                    GN._assert_column((k, ranks, kernel, what, j, "fs_pcgn"), X[:, j], infos[j], cs[j], Xs[:, j], N.Info(infos_s[j].iterations,
                                      infos_s[j].converged, infos_s[j].rnorm, infos_s[j].bnorm))
                    assert all(M.same_bits(cs[j][f], cs_s[j][f])[0] for f in N.PN), (k, ranks, kernel, j, cs[j], cs_s[j])
                assert st["iter"] == max(i.iterations for i in infos), (k, ranks, st)
        finally:
            dist.close()


def test_pcgn_more_than_one_grid_stride_capped(L):
    s = ALL["binary_F262145"]
    i = np.arange(s.ncol, dtype=np.float64)
    B = np.stack([s.b, np.cos(i * 0.013) + 0.5 * s.b], 1)
    single = _single_handles(L, s)
    dist = GC.Dist(L, s, 3, False)
    try:
        with options(strict_order=1):
            X, infos, _, cs = dpcgn(L, dist, s, B, P.PRECOND_JACOBI, max_iter=3)
            Xs, infos_s, _, _ = GN.pcgn_run(L, single[0], single[1], s, B, P.PRECOND_JACOBI, max_iter=3)
        for j in range(2):
            GN._assert_column((s.name, j), X[:, j], infos[j], cs[j], Xs[:, j], N.Info(infos_s[j].iterations, infos_s[j].converged,
                              infos_s[j].rnorm, infos_s[j].bnorm))
            assert infos[j].iterations == 3 and infos[j].converged == 0
    finally:
        dist.close()


def test_pcgn_warm_columns_freeze_at_different_iterations(L):
    s = ALL["valued"]
    i = np.arange(s.ncol, dtype=np.float64)
    B = np.stack([s.b, s.b * 0.5 + np.cos(i * 0.05), np.sin(i * 0.3) + 0.25 * s.b], 1)
    dist = GC.Dist(L, s, 3, True)
    try:
        with options(strict_order=1, dist_cg_scheme=0):
            X0 = np.zeros(B.shape)
            X0[:, 1] = dpcg(L, dist, s, P.PRECOND_JACOBI, max_iter=3, b=B[:, 1])[0]
            X0[:, 2] = dpcg(L, dist, s, P.PRECOND_JACOBI, tol=s.tol * 1e-2, b=B[:, 2])[0]
            alone = [dpcg(L, dist, s, P.PRECOND_JACOBI, x0=X0[:, j], b=B[:, j]) for j in range(3)]
            for kernel in GN.KERNELS:
                with options(pcgn_kernel=kernel):
                    X, infos, _, cs = dpcgn(L, dist, s, B, P.PRECOND_JACOBI, X0=X0)
                for j, (x, info, _) in enumerate(alone):
                    GN._assert_column((s.name, kernel, j), X[:, j], infos[j], cs[j], x, N.Info(info.iterations, info.converged, info.rnorm, info.bnorm))
        assert infos[2].iterations == 0 and infos[2].converged == 1 and M.same_bits(X[:, 2], X0[:, 2]).all()
        assert infos[0].iterations > infos[1].iterations > 0, [i.iterations for i in infos]
    finally:
        dist.close()


@pytest.mark.parametrize("mode", G.MODES)
def test_pcgn_one_column_is_fs_dist_pcg(L, mode):
    for name in ("scaled_seed0", "binary_F65", "valued", "zero_rhs"):
        s = ALL[name]
        dist = GC.Dist(L, s, 3, False)
        try:
            for case in (0, 1, 3):
                _, precond, x0, max_iter, diag = _case_args(s, case, s.t_csr_sorted())
                with GC._mode(mode), options(dist_cg_scheme=0):
                    x, info, st = dpcg(L, dist, s, precond, x0, max_iter, diag)
                    X, infos, stn, _ = dpcgn(L, dist, s, s.b.reshape(-1, 1), precond, None if x0 is None else x0.reshape(-1, 1), max_iter, diag)
                # (slots a solve never wrote hold what the allocation held in one and 0 in the other: the scalars every solve defines)
                want = {key: st[key] for key in ("done", "iter", "stop", "rr", "bb")}
                if info.iterations > 0 or info.converged == 0:
                    want.update(alpha=st["alpha"], rsq=st["rsq"])
                bad = M.mismatch(X[:, 0], x, infos[0].iterations, info.iterations, stn, want)
                assert bad is None, (name, mode, case, bad)
                assert infos[0].converged == info.converged and M.same_bits(infos[0].rnorm, info.rnorm)[0], (name, mode, case)
        finally:
            dist.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_statuses(L):
    from libfastsparse_amd import capi
    s = RECIPES0["scaled_seed0"]
    dist = GC.Dist(L, s, 3, False)
    rp, cc, vv = s.a_csr()
    M_not = L.fs_dist_csr_create(dist.D, s.nrow, s.ncol, len(cc), rp.ctypes.data, cc.ctypes.data, vv.ctypes.data)   # no transposed side
    assert M_not
    try:
        k = 3
        b, x, d = s.b.copy(), np.full(s.ncol, np.nan), G._caller_diag(s)
        B, X = GN.columns(s, k), np.full((s.ncol, k), np.nan)
        x_bits, X_bits = x.view(np.int64).copy(), X.view(np.int64).copy()

        def prm_of(kw):
            f = dict(tol=1e-8, max_iter=0, precond=P.PRECOND_JACOBI, warm_start=0, diag=None)
            f.update(kw)
            return C.byref(capi.PcgParams(f["tol"], f["max_iter"], f["precond"], f["warm_start"], f["diag"]))

        def one(M_=dist.M, x_=x.ctypes.data, b_=b.ctypes.data, prm="default", **kw):
            return L.fs_dist_pcg(M_, x_, b_, s.lam, prm_of(kw) if prm == "default" else prm, None)

        def many(M_=dist.M, X_=X.ctypes.data, B_=B.ctypes.data, k_=k, prm="default", **kw):
            return L.fs_dist_pcgn(M_, X_, B_, k_, s.lam, prm_of(kw) if prm == "default" else prm, None)

        for f, nm in ((one, "x_"), (many, "X_")):
            bad = {"NULL M": f(M_=None), "NULL x": f(**{nm: None}), "NULL b": f(**{"b_" if f is one else "B_": None}), "NULL prm": f(prm=None),
                   "precond 3": f(precond=3), "precond -1": f(precond=-1), "DIAG without diag": f(precond=P.PRECOND_DIAG),
                   "tol < 0": f(tol=-1e-8), "tol NaN": f(tol=float("nan")), "tol -inf": f(tol=float("-inf"))}
            assert all(rc == FS_ERR_ARG for rc in bad.values()), (f.__name__, bad)
            assert L.fs_last_error()
            assert f(M_=M_not) == FS_ERR_NO_TRANSPOSE, f.__name__
        assert {kk: many(k_=kk) for kk in (0, -1, N.MAX_RHS + 1)} == {0: FS_ERR_ARG, -1: FS_ERR_ARG, N.MAX_RHS + 1: FS_ERR_ARG}
        assert L.fs_dist_gram_diag(None, 0.0, x.ctypes.data) == FS_ERR_ARG and L.fs_dist_gram_diag(dist.M, 0.0, None) == FS_ERR_ARG
        assert L.fs_dist_gram_diag(M_not, 0.0, x.ctypes.data) == FS_ERR_NO_TRANSPOSE
        assert np.array_equal(x.view(np.int64), x_bits) and np.array_equal(X.view(np.int64), X_bits), "a refused call wrote to x / X"
        assert one(tol=0.0, max_iter=2) == FS_OK and many(tol=0.0, max_iter=2) == FS_OK      # tol = 0 with a cap, info NULL: legal
        assert one(precond=P.PRECOND_NONE, diag=d.ctypes.data, max_iter=1) == FS_OK          # diag is ignored unless FS_PRECOND_DIAG
    finally:
        L.fs_dist_matrix_destroy(M_not)
        dist.close()


def test_released_shard_of_the_transpose(L):
    """fs_matrix_release_csr on ONE rank's shard of A': Jacobi is refused before anything is written; a diagonal kept from before
    still solves, with the same bits"""
    from libfastsparse_amd import capi
    s = RECIPES0["scaled_seed0"]
    with options(binning=2, bin_flags=64):                           # kept two-pass copies: there is something to release for
        dist = GC.Dist(L, s, 3, False)
    try:
        kept = np.full(s.ncol, np.nan)
        capi.dist_gram_diag(dist.M, s.lam, kept)
        B = GN.columns(s, 2)
        before = {}
        for scheme in (0, 1):
            with options(dist_cg_scheme=scheme):
                before[scheme] = dpcg(L, dist, s, P.PRECOND_JACOBI)
                assert before[scheme][1].converged == 1
        X_before = dpcgn(L, dist, s, B, P.PRECOND_JACOBI)[0]
        assert L.fs_matrix_release_csr(L.fs_dist_matrix_shard(dist.M, 1, 1)) == 1
        prm = capi.PcgParams(s.tol, 0, P.PRECOND_JACOBI, 0, None)
        for scheme in (0, 1):
            with options(dist_cg_scheme=scheme):
                x, X, d = np.full(s.ncol, np.nan), np.full(B.shape, np.nan), np.full(s.ncol, np.nan)
                bits, Bits = x.view(np.int64).copy(), X.view(np.int64).copy()
                assert L.fs_dist_pcg(dist.M, x.ctypes.data, s.b.ctypes.data, s.lam, C.byref(prm), None) == FS_ERR_RELEASED
                assert b"fs_matrix_release_csr" in L.fs_last_error()
                assert L.fs_dist_pcgn(dist.M, X.ctypes.data, B.ctypes.data, 2, s.lam, C.byref(prm), None) == FS_ERR_RELEASED
                assert L.fs_dist_gram_diag(dist.M, s.lam, d.ctypes.data) == FS_ERR_RELEASED
                assert np.array_equal(x.view(np.int64), bits) and np.array_equal(X.view(np.int64), Bits) and np.isnan(d).all()
                x_diag, info_diag, _ = dpcg(L, dist, s, P.PRECOND_DIAG, diag=kept)   # Jacobi's own d, kept: the same dinv, the same bits
                assert info_diag.converged == 1 and info_diag.iterations == before[scheme][1].iterations, scheme
                assert M.same_bits(x_diag, before[scheme][0]).all(), scheme
        assert M.same_bits(dpcgn(L, dist, s, B, P.PRECOND_DIAG, diag=kept)[0], X_before).all()
    finally:
        dist.close()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
def test_guard_zones(L):
    """x, b, diag, X, B in HBM inside guard zones, 16-byte aligned and 8 bytes off: guards untouched, inputs unchanged"""
    import torch
    from libfastsparse_amd import capi
    mem = LC.TorchMem()
    s = RECIPES0["powerlaw_seed0"]
    k = 3
    diag, B = G._caller_diag(s), GN.columns(s, k).reshape(-1)
    dist = GC.Dist(L, s, 3, False)
    try:
        gx, gb, gd = LC.Guarded(mem, "x of fs_dist_pcg", s.ncol), LC.Guarded(mem, "b of fs_dist_pcg", s.ncol), LC.Guarded(mem, "diag of fs_dist_pcg", s.ncol)
        gX, gB = LC.Guarded(mem, "X of fs_dist_pcgn", s.ncol * k), LC.Guarded(mem, "B of fs_dist_pcgn", s.ncol * k)
        for scheme in (0, 1):
            for off in (0, 1):
                for what, precond, warm, max_iter in CASES:
                    mem.put(gb.place(s.ncol, off), s.b)
                    mem.put(gd.place(s.ncol, off ^ 1), diag)
                    mem.put(gB.place(s.ncol * k, off), B)
                    for g, n, x0 in ((gx, s.ncol, G._x0(s)), (gX, s.ncol * k, np.repeat(G._x0(s), k))):
                        if warm:
                            mem.put(g.place(n, off), x0)
                        else:
                            mem.fill_bits(g.place(n, off), LC.PREFILLS["nan"])
                    prm = capi.PcgParams(s.tol, max_iter, precond, int(warm), gd.view.data_ptr() if precond == P.PRECOND_DIAG else None)
                    info = capi.PcgInfo()
                    with options(dist_cg_scheme=scheme):
                        capi.check(L.fs_dist_pcg(dist.M, gx.view.data_ptr(), gb.view.data_ptr(), s.lam, C.byref(prm), C.byref(info)), "fs_dist_pcg")
                        if scheme == 0:
                            capi.check(L.fs_dist_pcgn(dist.M, gX.view.data_ptr(), gB.view.data_ptr(), k, s.lam, C.byref(prm), None), "fs_dist_pcgn")
                    torch.cuda.synchronize()
                    bad = mem.first_bad_guard([gx, gb, gd, gX, gB])
                    assert bad is None, (what, scheme, off, bad.first_broken())
                    assert mem.eq(gb.view, mem.const(s.b)) and mem.eq(gd.view, mem.const(diag)) and mem.eq(gB.view, mem.const(B)), (what, off, "an input changed")
                    assert np.isfinite(mem.get(gx.view)).all(), (what, scheme, off)
                    if scheme == 0:
                        assert np.isfinite(mem.get(gX.view)).all(), (what, off)
                    if not max_iter and precond != P.PRECOND_NONE:
                        assert info.converged == 1, (what, scheme, off, info.iterations)
        gdd = LC.Guarded(mem, "d of fs_dist_gram_diag", s.ncol)
        for off in (0, 1):
            mem.fill_bits(gdd.place(s.ncol, off), LC.PREFILLS["nan"])
            capi.dist_gram_diag(dist.M, s.lam, gdd.view)
            torch.cuda.synchronize()
            assert gdd.guards_ok(), (off, gdd.first_broken())
            assert M.same_bits(mem.get(gdd.view), P.gram_diag(s.t_csr_sorted(), s.lam)).all(), off
    finally:
        dist.close()


def test_interleaved_solves_share_the_work_space_and_give_it_back(L):
    """solves of different kinds interleaved on one handle keep their bits; after fs_dist_matrix_destroy free device memory is back
    where it was before the handle existed, within one solve's work space (the allowance of test_gpu_lifecycle.py's leak test)"""
    import torch
    s = RECIPES0["control_seed0"]
    B2, B5 = GN.columns(s, 2), GN.columns(s, 5)

    def kinds(dist):
        def with_scheme(scheme, f):
            def run():
                with options(dist_cg_scheme=scheme):
                    return f()
            return run
        y = np.full(s.nrow, np.nan)

        def spmv():
            assert L.fs_dist_spmv(dist.M, y.ctypes.data, s.b.ctypes.data) == 0
            return y.copy()
        return [with_scheme(0, lambda: dist.cg(False)[0]), with_scheme(0, lambda: dpcg(L, dist, s, P.PRECOND_JACOBI)[0]),
                with_scheme(1, lambda: dpcg(L, dist, s, P.PRECOND_JACOBI)[0]), lambda: dpcgn(L, dist, s, B2, P.PRECOND_JACOBI)[0],
                lambda: dpcgn(L, dist, s, B5, P.PRECOND_DIAG, diag=G._caller_diag(s), hbm=True)[0], spmv,
                with_scheme(1, lambda: dist.cg(False)[0]), with_scheme(1, lambda: dpcg(L, dist, s, P.PRECOND_DIAG, x0=G._x0(s), diag=G._caller_diag(s))[0])]

    def cycle(check):
        dist = GC.Dist(L, s, 3, False)
        try:
            fs = kinds(dist)
            first = [f() for f in fs]
            if check:
                order = np.random.default_rng(4).permutation(len(fs) * 2) % len(fs)
                for i in order:
                    assert M.same_bits(fs[i](), first[i]).all(), f"solve kind {i} changed its bits between other solves"
        finally:
            dist.close()

    cycle(True)                                                      # (warm-up: whatever the process keeps for good exists now)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    cycle(False)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    k = 5
    one_solve = 8 * (3 * k * s.ncol + k * s.nrow + s.ncol + 2048 * k + 512)
    print(f"free device memory: {free0} bytes before the handle, {free1} after its destroy; allowance {one_solve}")
    assert free0 - free1 <= one_solve, (free0, free1, one_solve)


# ---- 10 --------------------------------------------------------------------------------------------------------------------
# the three smallest systems of GC.DIST_SET (three unknowns on three ranks; tol = 0: every solve ends at its cap) and the seed0 recipes
PRODUCT_SET = ("three_eigenvalues", "cap_tol0", "fixture_100x50") + tuple(RECIPES0)


def _loops(cap, iterations, at_start=False):
    """iterations the host enqueues: the device sets `done` in loop iteration j and reports iterations == j; the host sees the flags of
    iteration j synchronously behind iteration j + 1, so j + 2 iterations were enqueued -- or the cap; none for a solve done at its start"""
    return 0 if at_start else min(cap, iterations + 2)


@pytest.mark.parametrize("name", PRODUCT_SET)
def test_sharded_products_per_solve(L, name):
    """fs_debug_dist_products() per solve, strict mode, three ranks: per_iter x min(cap, iterations + 2) + warm, with per_iter = 2 sharded
    products (replicate, fs_dist_pcgn, fs_dist_cg2) or 1 (gather: A' is the rank's own shard), and as many once in front of a warm start"""
    s = ALL[name]
    F = s.ncol
    dist = GC.Dist(L, s, 3, False)

    def counted(f):
        before = L.fs_debug_dist_products()
        out = f()
        return L.fs_debug_dist_products() - before, out

    try:
        for scheme, per_iter in ((0, 2), (1, 1)):
            with options(strict_order=1, dist_cg_scheme=scheme):
                n, (_, it, st) = counted(lambda: dist.cg(False))
                print(f"{name} scheme {scheme} fs_dist_cg: {n} products, {it} iterations, done {st['done']}")
                assert n == per_iter * _loops(F, it), (name, scheme, "fs_dist_cg", n, it)
                for precond in (P.PRECOND_NONE, P.PRECOND_JACOBI):
                    for x0 in (None, G._x0(s)):
                        for max_iter in (0, 2):
                            n, (x, info, _) = counted(lambda: dpcg(L, dist, s, precond, x0, max_iter))
                            start = np.zeros(F) if x0 is None else x0
                            at_start = info.converged == 1 and info.iterations == 0 and bool(M.same_bits(x, start).all())
                            what = (name, scheme, "fs_dist_pcg", precond, x0 is not None, max_iter, n, info.iterations, info.converged, at_start)
                            print(*what)
                            assert n == per_iter * (_loops(max_iter or F, info.iterations, at_start) + (x0 is not None)), what
                            assert at_start or max_iter or info.converged == 1 or info.iterations == F, what
                n, (x, info, _) = counted(lambda: dpcg(L, dist, s, P.PRECOND_JACOBI, b=np.zeros(F)))      # done at the start
                assert n == 0 and info.converged == 1 and info.iterations == 0, (name, scheme, n)
                if s.tol > 0.0:                                      # a warm start from a converged x: only the products in front
                    x1, info1, _ = dpcg(L, dist, s, P.PRECOND_JACOBI)
                    assert info1.converged == 1, (name, scheme)
                    n, (x2, info2, _) = counted(lambda: dpcg(L, dist, s, P.PRECOND_JACOBI, x0=x1, tol=s.tol * 10))
                    assert n == per_iter and info2.iterations == 0 and M.same_bits(x2, x1).all(), (name, scheme, n)
        with options(strict_order=1):
            for k in (1, 3):
                B = GN.columns(s, k)
                for X0, max_iter in ((None, 0), (GN.x0_columns(s, B), 2)):
                    n, (X, infos, st, _) = counted(lambda: dpcgn(L, dist, s, B, P.PRECOND_JACOBI, X0, max_iter))
                    start = np.zeros(B.shape) if X0 is None else X0
                    at_start = st["done"] == 1.0 and st["iter"] == 0.0 and bool(M.same_bits(X, start).all())
                    what = (name, "fs_dist_pcgn", k, X0 is not None, max_iter, n, st["iter"], st["done"], at_start)
                    print(*what)
                    assert st["iter"] == max(i.iterations for i in infos), what
                    assert n == 2 * (_loops(max_iter or F, int(st["iter"]), at_start) + (X0 is not None)), what
            if s.two:
                n, (_, it, st) = counted(lambda: dist.cg(True))
                print(f"{name} fs_dist_cg2: {n} products, {it} iterations")
                assert n == 2 * _loops(F, it), (name, "fs_dist_cg2", n, it)
    finally:
        dist.close()
