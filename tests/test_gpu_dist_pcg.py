"""fs_dist_gram_diag, fs_dist_pcg and fs_dist_pcgn on virtual ranks of one device (fs_dist_create(n, [0] * n)), against the CPU models
(tests/_pcg_model.py, _dist_pcg_model.py, _pcgn_model.py) and against the single-device solvers, on the harness of tests/_solvers.py and
tests/_dist_solvers.py.  A' of every model is dist.t_csr(): the shards' own rows, downloaded.

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
import contextlib
import ctypes as C

import numpy as np
import pytest

import _cg_model as M
import _dist_solvers as DV
import _gpu as G
import _lifecycle as LC
import _pcg_model as P
import _pcgn_model as N
import _solvers as SV
from _gpu import FS_ERR_ARG, FS_ERR_NO_TRANSPOSE, FS_ERR_RELEASED, FS_OK, L  # noqa: F401

pytestmark = pytest.mark.gpu

_MODELS = {}


def test_error_codes_are_the_header():
    import os
    with open(os.path.join(M.ROOT, "include", "fastsparse_hip.h")) as f:
        hdr = f.read()
    for name, v in (("FS_ERR_ARG", FS_ERR_ARG), ("FS_ERR_NO_TRANSPOSE", FS_ERR_NO_TRANSPOSE), ("FS_ERR_RELEASED", FS_ERR_RELEASED)):
        assert f"{name} = {v}" in " ".join(hdr.split()), name


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_t", [False, True], ids=["host-transpose", "device-transpose"])
@pytest.mark.parametrize("ranks", [1, 3, 5])
def test_gram_diag_is_fs_gram_diag(L, ranks, device_t):
    from libfastsparse_amd import capi
    for name, s in DV.ALL.items():
        dist = DV.Dist(L, s, ranks, device_t)
        try:
            t_csr = DV.sorted_t(dist, s)
            for lam in (s.lam, 0.0, 0.75):
                want = P.gram_diag(t_csr, lam)
                for hbm in (False, True):
                    d = G.put(np.full(s.ncol, np.nan), hbm)
                    capi.dist_gram_diag(dist.M, lam, d)
                    ok = M.same_bits(G.to_numpy(d), want)
                    assert ok.all(), (name, ranks, lam, hbm, int((~ok).sum()), int(np.flatnonzero(~ok)[0]))
                if lam == 0.0 and name == "lambda0_empty_column":
                    assert np.diff(t_csr[0])[5] == 0 and G.to_numpy(d)[5] == 0.0 and not np.signbit(G.to_numpy(d)[5])
            if ranks == 3 and not device_t:                          # fs_gram_diag on a single-device handle of the same CSR
                _, At = SV.single_handles(L, s)
                one = G.nan_vector(s.ncol)
                capi.gram_diag(At, s.lam, one, capi.current_stream())
                assert M.same_bits(one.cpu().numpy(), P.gram_diag(t_csr, s.lam)).all(), name
        finally:
            dist.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DV.ALL))
def test_scheme0_strict_is_fs_pcg(L, name):
    s = DV.ALL[name]
    single = {}
    for ranks, device_t in ((1, False), (3, False), (3, True), (1, True)):
        dist = DV.Dist(L, s, ranks, device_t)
        try:
            t_csr = DV.sorted_t(dist, s)
            with G.options(strict_order=1, dist_cg_scheme=0):
                for case in range(len(SV.CASES)):
                    what, precond, x0, max_iter, diag = DV.case_args(s, case, t_csr)
                    hbm = (case + ranks) % 2 == 1
                    x, info, st = DV.dpcg(L, dist, s, precond, x0, max_iter, diag, hbm=hbm)
                    model = DV.dpcg_model(s, case, t_csr)
                    entry = f"fs_dist_pcg scheme 0 {what}, {ranks} ranks, {'device' if device_t else 'host'} A', {'HBM' if hbm else 'host'} vectors"
                    bad = M.mismatch(x, model.x, info.iterations, model.iterations, st, model.state)
                    assert bad is None, f"{entry} on {name}: {bad}"
                    SV.assert_info((name, entry), info, model)
                    if ranks == 3 and not device_t:                  # a single-device fs_pcg on the same CSRs
                        if not single:
                            single["h"] = SV.single_handles(L, s)
                        xs, infos, _ = SV.pcg_run(L, single["h"][0], single["h"][1], s, precond, x0, max_iter, diag)
                        assert M.same_bits(x, xs).all() and (info.iterations, info.converged) == (infos.iterations, infos.converged), entry
                        assert M.same_bits(info.rnorm, infos.rnorm)[0] and M.same_bits(info.bnorm, infos.bnorm)[0], entry
                    if name == "zero_rhs" and x0 is None:
                        assert info.converged == 1 and info.iterations == 0 and M.same_bits(x, np.zeros(s.ncol)).all()
        finally:
            dist.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DV.ALL))
def test_scheme1_strict_is_the_slice_model(L, name):
    s = DV.ALL[name]
    for device_t in (False, True):
        dist = DV.Dist(L, s, 3, device_t)
        try:
            bounds = dist.bounds_t()
            assert bounds[0] == 0 and bounds[-1] == s.ncol
            t_csr = DV.sorted_t(dist, s)
            if name in DV.RECIPES0:                                     # on the CPU first: the slice tree is told from the whole one
                whole, sliced = DV.dpcg_model(s, 1, t_csr), DV.dpcg_model(s, 1, t_csr, bounds)
                differ = int((~M.same_bits(whole.x, sliced.x)).sum())
                print(f"{name} bounds {bounds}: {differ} of {s.ncol} entries differ between the slice model and the whole model")
                assert all(a < b for a, b in zip(bounds, bounds[1:])) and differ >= 1, (name, bounds, differ)
            with G.options(strict_order=1, dist_cg_scheme=1):
                for case in range(len(SV.CASES)):
                    what, precond, x0, max_iter, diag = DV.case_args(s, case, t_csr)
                    hbm = (case + int(device_t)) % 2 == 1
                    x, info, st = DV.dpcg(L, dist, s, precond, x0, max_iter, diag, hbm=hbm)
                    model = DV.dpcg_model(s, case, t_csr, bounds)
                    bad = M.mismatch(x, model.x, info.iterations, model.iterations, st, model.state)
                    assert bad is None, f"fs_dist_pcg scheme 1 {what}, bounds {bounds}, on {name}: {bad}"
                    SV.assert_info((name, what, bounds), info, model)
        finally:
            dist.close()


def test_scheme1_with_empty_slices(L):
    """five ranks on the three rows of A': some slices are empty and contribute +0.0"""
    s = DV.ALL["three_eigenvalues"]
    dist = DV.Dist(L, s, 5, False)
    try:
        bounds = dist.bounds_t()
        assert any(a == b for a, b in zip(bounds, bounds[1:])), bounds
        t_csr = DV.sorted_t(dist, s)
        with G.options(strict_order=1, dist_cg_scheme=1):
            for case in range(len(SV.CASES)):
                what, precond, x0, max_iter, diag = DV.case_args(s, case, t_csr)
                x, info, st = DV.dpcg(L, dist, s, precond, x0, max_iter, diag)
                model = DV.dpcg_model(s, case, t_csr, bounds)
                bad = M.mismatch(x, model.x, info.iterations, model.iterations, st, model.state)
                assert bad is None, f"fs_dist_pcg scheme 1 {what}, bounds {bounds}: {bad}"
    finally:
        dist.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in SV.RECIPES if n.startswith("scaled")])
def test_default_mode_jacobi_converges_where_plain_cg_does_not(L, name):
    s = SV.RECIPES[name]
    dist = DV.Dist(L, s, 3, False)
    try:
        DV.assert_default_mode_bars(L, dist, s)
    finally:
        dist.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_without_preconditioner_cold_is_fs_dist_cg(L, mode):
    for name, s in DV.ALL.items():
        dist = DV.Dist(L, s, 3, False)
        try:
            for scheme in (0, 1):
                with G.mode_options(mode), G.options(dist_cg_scheme=scheme):
                    xc, itc, stc = dist.cg(False)
                    x, info, st = DV.dpcg(L, dist, s)
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
    s = DV.RECIPES0["scaled_seed0"]
    dist = DV.Dist(L, s, 3, False)
    try:
        for scheme, in_front in ((0, 2), (1, 1)):
            with G.options(dist_cg_scheme=scheme):
                before = L.fs_debug_dist_products()
                x, info, _ = DV.dpcg(L, dist, s, P.PRECOND_JACOBI, b=np.zeros(s.ncol))
                assert L.fs_debug_dist_products() == before, scheme
                assert info.converged == 1 and info.iterations == 0 and info.bnorm == 0.0 and M.same_bits(x, np.zeros(s.ncol)).all()
                x1, info1, _ = DV.dpcg(L, dist, s, P.PRECOND_JACOBI, tol=s.tol)
                assert info1.converged == 1 and info1.iterations > 0
                before = L.fs_debug_dist_products()
                x2, info2, _ = DV.dpcg(L, dist, s, P.PRECOND_JACOBI, x0=x1, tol=s.tol * 10)
                assert L.fs_debug_dist_products() - before == in_front, (scheme, L.fs_debug_dist_products() - before)
                assert info2.converged == 1 and info2.iterations == 0 and M.same_bits(x2, x1).all(), scheme
        B = SV.columns(s, 3)
        before = L.fs_debug_dist_products()
        X, infos, _, _ = DV.dpcgn(L, dist, s, np.zeros_like(B), P.PRECOND_JACOBI)
        assert L.fs_debug_dist_products() == before and all(i.converged == 1 and i.iterations == 0 for i in infos)
        assert M.same_bits(X, np.zeros_like(B)).all()
    finally:
        dist.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", DV.KS)
def test_pcgn_columns_are_fs_pcgn_and_the_model(L, k):
    s, B = DV.panel(k)
    case = k % len(SV.CASES)
    single = SV.single_handles(L, s)
    for ranks in (1, 3):
        dist = DV.Dist(L, s, ranks, ranks == 3)
        try:
            t_csr = DV.sorted_t(dist, s)
            what, precond, x0, max_iter, diag = DV.case_args(s, case, t_csr)
            X0 = SV.x0_columns(s, B) if x0 is not None else None
            am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr)
            dinv = None if precond == P.PRECOND_NONE else P.dinv_of(P.gram_diag(t_csr, s.lam) if precond == P.PRECOND_JACOBI else diag)
            key = ("pcgn", k, case)
            if key not in _MODELS:
                _MODELS[key] = N.pcgn(s.ncol, am, atm, B, s.lam, s.tol, max_iter, dinv, X0)
            model = _MODELS[key]
            for kernel in ((1, 2) if k > 4 else (0,)):
                with G.options(strict_order=1, pcgn_kernel=kernel):
                    X, infos, st, cs = DV.dpcgn(L, dist, s, B, precond, X0, max_iter, diag, hbm=ranks == 3)
                    Xs, infos_s, _, cs_s = SV.pcgn_run(L, single[0], single[1], s, B, precond, X0, max_iter, diag)
                    with G.options(dist_cg_scheme=1):                  # replicated whatever the scheme says
                        X1, infos1, _, _ = DV.dpcgn(L, dist, s, B, precond, X0, max_iter, diag)
                assert len(infos) == k
                assert M.same_bits(X1, X).all() and [i.iterations for i in infos1] == [i.iterations for i in infos], (k, ranks, kernel)
                for j in range(k):
                    SV.assert_column((k, ranks, kernel, what, j, "model"), X[:, j], infos[j], cs[j], model.X[:, j], model.infos[j], model.columns[j].state)
                    SV.assert_column((k, ranks, kernel, what, j, "fs_pcgn"), X[:, j], infos[j], cs[j], Xs[:, j], N.Info(infos_s[j].iterations,
                                      infos_s[j].converged, infos_s[j].rnorm, infos_s[j].bnorm))
                    assert all(M.same_bits(cs[j][f], cs_s[j][f])[0] for f in N.PN), (k, ranks, kernel, j, cs[j], cs_s[j])
                assert st["iter"] == max(i.iterations for i in infos), (k, ranks, st)
        finally:
            dist.close()


def test_pcgn_more_than_one_grid_stride_capped(L):
    s = DV.ALL["binary_F262145"]
    i = np.arange(s.ncol, dtype=np.float64)
    B = np.stack([s.b, np.cos(i * 0.013) + 0.5 * s.b], 1)
    single = SV.single_handles(L, s)
    dist = DV.Dist(L, s, 3, False)
    try:
        with G.options(strict_order=1):
            X, infos, _, cs = DV.dpcgn(L, dist, s, B, P.PRECOND_JACOBI, max_iter=3)
            Xs, infos_s, _, _ = SV.pcgn_run(L, single[0], single[1], s, B, P.PRECOND_JACOBI, max_iter=3)
        for j in range(2):
            SV.assert_column((s.name, j), X[:, j], infos[j], cs[j], Xs[:, j], N.Info(infos_s[j].iterations, infos_s[j].converged,
                              infos_s[j].rnorm, infos_s[j].bnorm))
            assert infos[j].iterations == 3 and infos[j].converged == 0
    finally:
        dist.close()


def test_pcgn_warm_columns_freeze_at_different_iterations(L):
    s = DV.ALL["valued"]
    i = np.arange(s.ncol, dtype=np.float64)
    B = np.stack([s.b, s.b * 0.5 + np.cos(i * 0.05), np.sin(i * 0.3) + 0.25 * s.b], 1)
    dist = DV.Dist(L, s, 3, True)
    try:
        with G.options(strict_order=1, dist_cg_scheme=0):
            X0 = np.zeros(B.shape)
            X0[:, 1] = DV.dpcg(L, dist, s, P.PRECOND_JACOBI, max_iter=3, b=B[:, 1])[0]
            X0[:, 2] = DV.dpcg(L, dist, s, P.PRECOND_JACOBI, tol=s.tol * 1e-2, b=B[:, 2])[0]
            alone = [DV.dpcg(L, dist, s, P.PRECOND_JACOBI, x0=X0[:, j], b=B[:, j]) for j in range(3)]
            for kernel in SV.KERNELS:
                with G.options(pcgn_kernel=kernel):
                    X, infos, _, cs = DV.dpcgn(L, dist, s, B, P.PRECOND_JACOBI, X0=X0)
                for j, (x, info, _) in enumerate(alone):
                    SV.assert_column((s.name, kernel, j), X[:, j], infos[j], cs[j], x, N.Info(info.iterations, info.converged, info.rnorm, info.bnorm))
        assert infos[2].iterations == 0 and infos[2].converged == 1 and M.same_bits(X[:, 2], X0[:, 2]).all()
        assert infos[0].iterations > infos[1].iterations > 0, [i.iterations for i in infos]
    finally:
        dist.close()


@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_pcgn_one_column_is_fs_dist_pcg(L, mode):
    for name in ("scaled_seed0", "binary_F65", "valued", "zero_rhs"):
        s = DV.ALL[name]
        dist = DV.Dist(L, s, 3, False)
        try:
            for case in (0, 1, 3):
                _, precond, x0, max_iter, diag = DV.case_args(s, case, s.t_csr_sorted())
                with G.mode_options(mode), G.options(dist_cg_scheme=0):
                    x, info, st = DV.dpcg(L, dist, s, precond, x0, max_iter, diag)
                    X, infos, stn, _ = DV.dpcgn(L, dist, s, s.b.reshape(-1, 1), precond, None if x0 is None else x0.reshape(-1, 1), max_iter, diag)
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
    s = DV.RECIPES0["scaled_seed0"]
    with contextlib.closing(DV.Dist(L, s, 3, False)) as dist, DV.handle_without_transpose(L, dist, s) as M_not:
        k = 3
        b, x, d = s.b.copy(), np.full(s.ncol, np.nan), SV.caller_diag(s)
        B, X = SV.columns(s, k), np.full((s.ncol, k), np.nan)
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


def test_released_shard_of_the_transpose(L):
    """fs_matrix_release_csr on ONE rank's shard of A': Jacobi is refused before anything is written; a diagonal kept from before
    still solves, with the same bits"""
    from libfastsparse_amd import capi
    s = DV.RECIPES0["scaled_seed0"]
    with G.options(binning=2, bin_flags=64):                           # kept two-pass copies: there is something to release for
        dist = DV.Dist(L, s, 3, False)
    try:
        kept = np.full(s.ncol, np.nan)
        capi.dist_gram_diag(dist.M, s.lam, kept)
        B = SV.columns(s, 2)
        before = {}
        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                before[scheme] = DV.dpcg(L, dist, s, P.PRECOND_JACOBI)
                assert before[scheme][1].converged == 1
        X_before = DV.dpcgn(L, dist, s, B, P.PRECOND_JACOBI)[0]
        assert L.fs_matrix_release_csr(L.fs_dist_matrix_shard(dist.M, 1, 1)) == 1
        prm = capi.PcgParams(s.tol, 0, P.PRECOND_JACOBI, 0, None)
        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                x, X, d = np.full(s.ncol, np.nan), np.full(B.shape, np.nan), np.full(s.ncol, np.nan)
                bits, Bits = x.view(np.int64).copy(), X.view(np.int64).copy()
                assert L.fs_dist_pcg(dist.M, x.ctypes.data, s.b.ctypes.data, s.lam, C.byref(prm), None) == FS_ERR_RELEASED
                assert b"fs_matrix_release_csr" in L.fs_last_error()
                assert L.fs_dist_pcgn(dist.M, X.ctypes.data, B.ctypes.data, 2, s.lam, C.byref(prm), None) == FS_ERR_RELEASED
                assert L.fs_dist_gram_diag(dist.M, s.lam, d.ctypes.data) == FS_ERR_RELEASED
                assert np.array_equal(x.view(np.int64), bits) and np.array_equal(X.view(np.int64), Bits) and np.isnan(d).all()
                x_diag, info_diag, _ = DV.dpcg(L, dist, s, P.PRECOND_DIAG, diag=kept)   # Jacobi's own d, kept: the same dinv, the same bits
                assert info_diag.converged == 1 and info_diag.iterations == before[scheme][1].iterations, scheme
                assert M.same_bits(x_diag, before[scheme][0]).all(), scheme
        assert M.same_bits(DV.dpcgn(L, dist, s, B, P.PRECOND_DIAG, diag=kept)[0], X_before).all()
    finally:
        dist.close()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
def test_guard_zones(L):
    """x, b, diag, X, B in HBM inside guard zones, 16-byte aligned and 8 bytes off: guards untouched, inputs unchanged"""
    import torch
    from libfastsparse_amd import capi
    mem = LC.TorchMem()
    s = DV.RECIPES0["powerlaw_seed0"]
    k = 3
    diag, B = SV.caller_diag(s), SV.columns(s, k).reshape(-1)
    dist = DV.Dist(L, s, 3, False)
    try:
        gx, gb, gd = LC.Guarded(mem, "x of fs_dist_pcg", s.ncol), LC.Guarded(mem, "b of fs_dist_pcg", s.ncol), LC.Guarded(mem, "diag of fs_dist_pcg", s.ncol)
        gX, gB = LC.Guarded(mem, "X of fs_dist_pcgn", s.ncol * k), LC.Guarded(mem, "B of fs_dist_pcgn", s.ncol * k)
        for scheme in (0, 1):
            for off in (0, 1):
                for what, precond, warm, max_iter in SV.CASES:
                    mem.put(gb.place(s.ncol, off), s.b)
                    mem.put(gd.place(s.ncol, off ^ 1), diag)
                    mem.put(gB.place(s.ncol * k, off), B)
                    for g, n, x0 in ((gx, s.ncol, SV.x0(s)), (gX, s.ncol * k, np.repeat(SV.x0(s), k))):
                        if warm:
                            mem.put(g.place(n, off), x0)
                        else:
                            mem.fill_bits(g.place(n, off), LC.PREFILLS["nan"])
                    prm = capi.PcgParams(s.tol, max_iter, precond, int(warm), gd.view.data_ptr() if precond == P.PRECOND_DIAG else None)
                    info = capi.PcgInfo()
                    with G.options(dist_cg_scheme=scheme):
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
    s = DV.RECIPES0["control_seed0"]
    B2, B5 = SV.columns(s, 2), SV.columns(s, 5)

    def kinds(dist):
        y = np.full(s.nrow, np.nan)

        def spmv():
            assert L.fs_dist_spmv(dist.M, y.ctypes.data, s.b.ctypes.data) == 0
            return y.copy()
        return [DV.with_scheme(0, lambda: dist.cg(False)[0]), DV.with_scheme(0, lambda: DV.dpcg(L, dist, s, P.PRECOND_JACOBI)[0]),
                DV.with_scheme(1, lambda: DV.dpcg(L, dist, s, P.PRECOND_JACOBI)[0]), lambda: DV.dpcgn(L, dist, s, B2, P.PRECOND_JACOBI)[0],
                lambda: DV.dpcgn(L, dist, s, B5, P.PRECOND_DIAG, diag=SV.caller_diag(s), hbm=True)[0], spmv,
                DV.with_scheme(1, lambda: dist.cg(False)[0]), DV.with_scheme(1, lambda: DV.dpcg(L, dist, s, P.PRECOND_DIAG, x0=SV.x0(s), diag=SV.caller_diag(s))[0])]

    k = 5
    one_solve = 8 * (3 * k * s.ncol + k * s.nrow + s.ncol + 2048 * k + 512)
    DV.interleaved_then_memory_back(L, s, 3, kinds, 4, one_solve)


# ---- 10 --------------------------------------------------------------------------------------------------------------------
# the three smallest systems of SV.DIST_SET (three unknowns on three ranks; tol = 0: every solve ends at its cap) and the seed0 recipes
PRODUCT_SET = ("three_eigenvalues", "cap_tol0", "fixture_100x50") + tuple(DV.RECIPES0)


@pytest.mark.parametrize("name", PRODUCT_SET)
def test_sharded_products_per_solve(L, name):
    """fs_debug_dist_products() per solve, strict mode, three ranks: per_iter x min(cap, iterations + 2) + warm, with per_iter = 2 sharded
    products (replicate, fs_dist_pcgn, fs_dist_cg2) or 1 (gather: A' is the rank's own shard), and as many once in front of a warm start"""
    s = DV.ALL[name]
    F = s.ncol
    dist = DV.Dist(L, s, 3, False)
    try:
        for scheme, per_iter in ((0, 2), (1, 1)):
            with G.options(strict_order=1, dist_cg_scheme=scheme):
                n, (_, it, st) = DV.counted(L, lambda: dist.cg(False))
                print(f"{name} scheme {scheme} fs_dist_cg: {n} products, {it} iterations, done {st['done']}")
                assert n == per_iter * DV.loops(F, it), (name, scheme, "fs_dist_cg", n, it)
                for precond in (P.PRECOND_NONE, P.PRECOND_JACOBI):
                    for x0 in (None, SV.x0(s)):
                        for max_iter in (0, 2):
                            n, (x, info, _) = DV.counted(L, lambda: DV.dpcg(L, dist, s, precond, x0, max_iter))
                            start = np.zeros(F) if x0 is None else x0
                            at_start = info.converged == 1 and info.iterations == 0 and bool(M.same_bits(x, start).all())
                            what = (name, scheme, "fs_dist_pcg", precond, x0 is not None, max_iter, n, info.iterations, info.converged, at_start)
                            print(*what)
                            assert n == per_iter * (DV.loops(max_iter or F, info.iterations, at_start) + (x0 is not None)), what
                            assert at_start or max_iter or info.converged == 1 or info.iterations == F, what
                n, (x, info, _) = DV.counted(L, lambda: DV.dpcg(L, dist, s, P.PRECOND_JACOBI, b=np.zeros(F)))      # done at the start
                assert n == 0 and info.converged == 1 and info.iterations == 0, (name, scheme, n)
                if s.tol > 0.0:                                      # a warm start from a converged x: only the products in front
                    x1, info1, _ = DV.dpcg(L, dist, s, P.PRECOND_JACOBI)
                    assert info1.converged == 1, (name, scheme)
                    n, (x2, info2, _) = DV.counted(L, lambda: DV.dpcg(L, dist, s, P.PRECOND_JACOBI, x0=x1, tol=s.tol * 10))
                    assert n == per_iter and info2.iterations == 0 and M.same_bits(x2, x1).all(), (name, scheme, n)
        with G.options(strict_order=1):
            for k in (1, 3):
                B = SV.columns(s, k)
                for X0, max_iter in ((None, 0), (SV.x0_columns(s, B), 2)):
                    n, (X, infos, st, _) = DV.counted(L, lambda: DV.dpcgn(L, dist, s, B, P.PRECOND_JACOBI, X0, max_iter))
                    start = np.zeros(B.shape) if X0 is None else X0
                    at_start = st["done"] == 1.0 and st["iter"] == 0.0 and bool(M.same_bits(X, start).all())
                    what = (name, "fs_dist_pcgn", k, X0 is not None, max_iter, n, st["iter"], st["done"], at_start)
                    print(*what)
                    assert st["iter"] == max(i.iterations for i in infos), what
                    assert n == 2 * (DV.loops(max_iter or F, int(st["iter"]), at_start) + (X0 is not None)), what
            if s.two:
                n, (_, it, st) = DV.counted(L, lambda: dist.cg(True))
                print(f"{name} fs_dist_cg2: {n} products, {it} iterations")
                assert n == 2 * DV.loops(F, it), (name, "fs_dist_cg2", n, it)
    finally:
        dist.close()
