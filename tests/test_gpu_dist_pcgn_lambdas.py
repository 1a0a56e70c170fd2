"""fs_dist_pcgn_lambdas on virtual ranks of one device (fs_dist_create(n, [0] * n)), against the CPU model
(tests/_dist_pcgn_lambdas_model.py: column j is the model of fs_dist_pcg at lambda_j), against fs_pcgn_lambdas on one device and
against fs_dist_pcgn / fs_dist_pcg, on the harness of tests/_solvers.py and tests/_dist_solvers.py.  A' of every model is
dist.t_csr(): the shards' own rows, downloaded.

1  strict_order, scheme 0, on 1 and 3 ranks, A' built on the host and on the device: the model's bits and those of a single-device
   fs_pcgn_lambdas on the same CSRs -- k in (1, 2, 3, 4, 5, 8, 17, 32), the cases of _solvers.CASES, both forms of the kernels for
   k > 4, X in host memory and in HBM.
2  strict_order, scheme 1 on three ranks: the slice model on bounds_t(), which is first shown, on the CPU, to differ from the whole
   model in at least half of the non-zero columns; five ranks on three unknowns leave empty slices.
3  F = 262145 on three ranks (more than one grid stride per whole panel, slices of 87 381 rows), cap 3, both schemes: k = 2 (a lane
   per row) and k = 17 staged.
4  equal lambdas are fs_dist_pcgn under scheme 0 and k = 1 is fs_dist_pcg at that lambda under both schemes, in every mode.
5  a ladder whose large rungs freeze early, on slices: a frozen column is not written again.
6  default mode, eight rungs on the column-scaled and the power-law recipe, both schemes: converged, true residual <= 2 tol, repeats.
7  sharded products per solve: 2 per iteration under scheme 0, 1 under scheme 1, as many in front of a warm start, none for a solve
   done at its start.
8  statuses, with X untouched by every refused call; a released shard of A'.
9  guard zones, interleaved solves on one handle, device memory given back.
10 a pair handle: both schemes are the models on the caller's A' order and cuts."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import _cg_model as M
import _dist_pair as DPair
import _dist_pcgn_lambdas_model as DNL
import _dist_solvers as DV
import _gpu as G
import _lifecycle as LC
import _pcg_model as P
import _pcgn_lambdas_model as NL
import _pcgn_model as N
import _solvers as SV
from _gpu import FS_ERR_ARG, FS_ERR_NO_TRANSPOSE, FS_ERR_RELEASED, FS_OK, L  # noqa: F401

pytestmark = pytest.mark.gpu

NONE, JACOBI, DIAG = P.PRECOND_NONE, P.PRECOND_JACOBI, P.PRECOND_DIAG


def _case(s, B, case, t_csr):
    what, precond, warm, max_iter = SV.CASES[case]
    diag = None
    if precond == DIAG:
        diag = np.abs(P.gram_diag(t_csr, s.lam)) * (1.0 + 0.5 * np.cos(np.arange(s.ncol) * 1.7)) + 0.125
    return what, precond, (SV.x0_columns(s, B) if warm else None), max_iter, diag


def _model(s, B, lams, precond, X0, max_iter, diag, t_csr, bounds=None):
    return DNL.run(s, B, lams, precond, max_iter=max_iter, X0=X0, diag=diag, t_csr=t_csr, bounds=bounds, cache=DV.DNL_CACHE)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", DV.KS)
def test_scheme0_strict_is_fs_pcgn_lambdas_and_the_model(L, k):
    s, B = DV.panel(k)
    lams = NL.rungs(s, k)
    case = k % len(SV.CASES)
    single = SV.single_handles(L, s)
    for ranks, device_t in ((1, False), (3, True), (3, False)):
        dist = DV.Dist(L, s, ranks, device_t)
        try:
            t_csr = DV.sorted_t(dist, s)
            what, precond, X0, max_iter, diag = _case(s, B, case, t_csr)
            model = _model(s, B, lams, precond, X0, max_iter, diag, t_csr)
            for kernel in ((1, 2) if k > 4 else (0,)):
                with G.options(strict_order=1, pcgn_kernel=kernel, dist_cg_scheme=0):
                    got = DV.dnl(L, dist, s, B, lams, precond, X0, max_iter, diag, hbm=(ranks == 3) != device_t)
                    one = SV.lambdas_run(L, single[0], single[1], s, B, lams, precond, X0, max_iter, diag)
                entry = (k, what, ranks, device_t, kernel)
                assert len(got[1]) == k
                DV.assert_dnl_model(entry, got, model)
                SV.same_solve(entry + ("fs_pcgn_lambdas",), got, one)
                assert (got[2]["done"], got[2]["iter"]) == (one[2]["done"], one[2]["iter"]), (entry, got[2], one[2])
        finally:
            dist.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", DV.KS)
def test_scheme1_strict_is_the_slice_model(L, k):
    s, B = DV.panel(k)
    lams = NL.rungs(s, k)
    case = k % len(SV.CASES)
    for device_t in (False, True):
        dist = DV.Dist(L, s, 3, device_t)
        try:
            bounds = dist.bounds_t()
            assert bounds[0] == 0 and bounds[-1] == s.ncol and all(a < b for a, b in zip(bounds, bounds[1:]))
            t_csr = DV.sorted_t(dist, s)
            what, precond, X0, max_iter, diag = _case(s, B, case, t_csr)
            whole = _model(s, B, lams, precond, X0, max_iter, diag, t_csr)
            sliced = _model(s, B, lams, precond, X0, max_iter, diag, t_csr, bounds)
            nz = SV.nonzero_columns(B)                                 # on the CPU first: the slice tree is told from the whole one
            differ = [j for j in nz if not M.same_bits(whole.X[:, j], sliced.X[:, j]).all()]
            print(f"k {k} {what} bounds {bounds}: {len(differ)} of {len(nz)} non-zero columns differ between the slice model and the whole model")
            assert 2 * len(differ) >= len(nz), (k, what, bounds, differ)
            for kernel in ((1, 2) if k > 4 else (0,)):
                with G.options(strict_order=1, pcgn_kernel=kernel, dist_cg_scheme=1):
                    got = DV.dnl(L, dist, s, B, lams, precond, X0, max_iter, diag, hbm=device_t)
                DV.assert_dnl_model((k, what, device_t, kernel, "slices"), got, sliced)
        finally:
            dist.close()


def test_scheme1_with_empty_slices(L):
    s = DV.ALL["three_eigenvalues"]
    dist = DV.Dist(L, s, 5, False)
    try:
        bounds = dist.bounds_t()
        assert len(bounds) == 6 and any(a == b for a, b in zip(bounds, bounds[1:])), bounds
        t_csr = DV.sorted_t(dist, s)
        for k in (1, 3, 8):
            B = SV.columns(s, k)
            lams = NL.rungs(s, k)
            for case in (0, 1, 3):
                what, precond, X0, max_iter, diag = _case(s, B, case, t_csr)
                model = _model(s, B, lams, precond, X0, max_iter, diag, t_csr, bounds)
                for kernel in SV.KERNELS:
                    with G.options(strict_order=1, pcgn_kernel=kernel, dist_cg_scheme=1):
                        got = DV.dnl(L, dist, s, B, lams, precond, X0, max_iter, diag)
                    DV.assert_dnl_model((k, what, kernel, bounds), got, model)
    finally:
        dist.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,kernel", [(2, 1), (17, 2)])
def test_large_slices_capped(L, k, kernel):
    s = DV.ALL["binary_F262145"]
    F = s.ncol
    i = np.arange(F, dtype=np.float64)
    B = np.ascontiguousarray(np.stack([s.b * (1.0 + 0.125 * j) + np.cos(i * (0.013 + 0.002 * j)) * (j > 0) for j in range(k)], 1))
    lams = NL.rungs(s, k)
    checked = [j for j in (0, 8, 16) if j < k] if k > 2 else [0, 1]
    # (a workgroup owns 256 rows whatever the height of a staged tile, so the grid stride is 262 144 rows for both forms of the
    #  kernels: the whole panel of scheme 0 runs into a second stride, a slice of a third of it runs many staged tiles per workgroup)
    assert F > M.RED_BLOCKS * M.RED_THREADS
    dist = DV.Dist(L, s, 3, False)
    try:
        bounds = dist.bounds_t()
        assert min(b - a for a, b in zip(bounds, bounds[1:])) > 65536, bounds
        t_csr = DV.sorted_t(dist, s)
        for scheme in (0, 1):
            with G.options(strict_order=1, pcgn_kernel=kernel, dist_cg_scheme=scheme):
                got = DV.dnl(L, dist, s, B, lams, JACOBI, max_iter=3, hbm=scheme == 1)
            model = _model(s, B[:, checked], [lams[j] for j in checked], JACOBI, None, 3, None, t_csr, bounds if scheme == 1 else None)
            X, infos, _, cs = got
            assert np.isfinite(X).all(), (k, scheme)
            for at, j in enumerate(checked):
                SV.assert_column((k, scheme, j), X[:, j], infos[j], cs[j], model.X[:, at], model.infos[at], model.columns[at].state)
            assert all(i.iterations <= 3 for i in infos) and (infos[0].iterations, infos[0].converged) == (3, 0), [(i.iterations, i.converged) for i in infos]
    finally:
        dist.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_equal_lambdas_are_fs_dist_pcgn(L, mode):
    s = DV.ALL["valued"]
    dist = DV.Dist(L, s, 3, False)
    try:
        for k in (1, 4, 8, 17):
            B = SV.columns(s, k)
            for precond, X0 in ((JACOBI, None), (NONE, None), (JACOBI, SV.x0_columns(s, B))):
                with G.mode_options(mode), G.options(dist_cg_scheme=0):
                    want = DV.dpcgn(L, dist, s, B, precond, X0)
                    got = DV.dnl(L, dist, s, B, [s.lam] * k, precond, X0)
                SV.same_solve((mode, k, precond, X0 is not None), got, want)
                assert all(i.converged == 1 for i in got[1])
    finally:
        dist.close()


@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_one_column_is_fs_dist_pcg_at_its_lambda(L, mode):
    from libfastsparse_amd import capi
    for name in ("scaled_seed0", "binary_F65", "valued", "zero_rhs"):
        s = DV.ALL[name]
        lam = NL.rungs(s, 2)[1]
        dist = DV.Dist(L, s, 3, False)
        try:
            for scheme in (0, 1):
                for case in (0, 1, 3):
                    _, precond, x0, max_iter, diag = DV.case_args(s, case, s.t_csr_sorted())
                    with G.mode_options(mode), G.options(dist_cg_scheme=scheme):
                        x = np.full(s.ncol, np.nan) if x0 is None else x0.copy()
                        info = capi.dist_pcg(dist.M, x, s.b.copy(), lam, s.tol, max_iter=max_iter, precond=precond, warm_start=x0 is not None, diag=diag)
                        st = P.state_from_device(SV.raw_state(L))
                        X, infos, stn, _ = DV.dnl(L, dist, s, s.b.reshape(-1, 1), [lam], precond, None if x0 is None else x0.reshape(-1, 1), max_iter, diag)
                    want = {key: st[key] for key in ("done", "iter", "stop", "rr", "bb")}
                    if info.iterations > 0 or info.converged == 0:
                        want.update(alpha=st["alpha"], rsq=st["rsq"])
                    bad = M.mismatch(X[:, 0], x, infos[0].iterations, info.iterations, stn, want)
                    assert bad is None, (name, mode, scheme, case, bad)
                    assert infos[0].converged == info.converged and M.same_bits(infos[0].rnorm, info.rnorm)[0], (name, mode, scheme, case)
        finally:
            dist.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_frozen_columns_are_not_written_again(L):
    s = SV.RECIPES["powerlaw_seed0"]
    lams = NL.rungs(s, 8)
    assert max(lams) == 1e6 * s.lam
    B = np.ascontiguousarray(np.repeat(s.b[:, None], 8, 1))
    dist = DV.Dist(L, s, 3, False)
    try:
        bounds = dist.bounds_t()
        t_csr = DV.sorted_t(dist, s)
        model = _model(s, B, lams, JACOBI, None, 0, None, t_csr, bounds)
        counts = [i.iterations for i in model.infos]
        assert len(set(counts)) >= 3 and counts[7] + 2 < max(counts), counts
        for kernel in SV.KERNELS:
            with G.options(strict_order=1, pcgn_kernel=kernel, dist_cg_scheme=1):
                got = DV.dnl(L, dist, s, B, lams, JACOBI)
                DV.assert_dnl_model(("ladder", kernel), got, model)
                for j in (7, 5, 3):                                  # the solve capped where column j froze: that column is final there
                    capped = DV.dnl(L, dist, s, B, lams, JACOBI, max_iter=counts[j] + 1)
                    assert capped[1][j].converged == 1 and capped[1][j].iterations == counts[j], (j, capped[1][j].iterations)
                    assert M.same_bits(capped[0][:, j], got[0][:, j]).all(), (kernel, j, "a frozen column was written again")
                    assert capped[2]["iter"] <= counts[j] + 1
    finally:
        dist.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("scaled_seed0", "powerlaw_seed0"))
def test_default_mode_ladder_converges_and_repeats(L, name):
    s = SV.RECIPES[name]
    lams = NL.rungs(s, 8)
    B = np.ascontiguousarray(np.repeat(s.b[:, None], 8, 1))
    A = P.dense(s)
    Gm = A.T @ A
    dist = DV.Dist(L, s, 3, False)
    try:
        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                first, again = [DV.dnl(L, dist, s, B, lams, JACOBI, hbm=bool(run)) for run in range(2)]
            SV.same_solve((name, scheme, "a second solve repeats the bits"), again, first)
            X, infos, _, _ = first
            for j, lam in enumerate(lams):
                assert infos[j].converged == 1, (name, scheme, j, infos[j].iterations)
                res = float(np.linalg.norm((Gm + lam * np.eye(s.ncol)) @ X[:, j] - s.b) / np.linalg.norm(s.b))
                assert res <= 2 * s.tol, (name, scheme, j, lam, res)
                assert infos[j].rnorm <= s.tol * infos[j].bnorm, (name, scheme, j)
    finally:
        dist.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("three_eigenvalues", "fixture_100x50", "scaled_seed0"))
def test_sharded_products_per_solve(L, name):
    s = DV.ALL[name]
    F = s.ncol
    dist = DV.Dist(L, s, 3, False)
    try:
        for scheme, per_iter in ((0, 2), (1, 1)):
            with G.options(strict_order=1, dist_cg_scheme=scheme):
                for k in (1, 3):
                    B = SV.columns(s, k)
                    lams = NL.rungs(s, k)
                    for X0, max_iter in ((None, 0), (SV.x0_columns(s, B), 2)):
                        n, (X, infos, st, _) = DV.counted(L, lambda: DV.dnl(L, dist, s, B, lams, JACOBI, X0, max_iter))
                        start = np.zeros(B.shape) if X0 is None else X0
                        at_start = st["done"] == 1.0 and st["iter"] == 0.0 and bool(M.same_bits(X, start).all())
                        what = (name, scheme, k, X0 is not None, max_iter, n, st["iter"], st["done"], at_start)
                        print(*what)
                        assert st["iter"] == max(i.iterations for i in infos), what
                        assert n == per_iter * (DV.loops(max_iter or F, int(st["iter"]), at_start) + (X0 is not None)), what
                    n, (X, infos, _, _) = DV.counted(L, lambda: DV.dnl(L, dist, s, np.zeros_like(B), lams, JACOBI, tol=1.0))   # done at the start
                    assert n == 0 and all(i.converged == 1 and i.iterations == 0 for i in infos), (name, scheme, k, n)
                    assert M.same_bits(X, np.zeros_like(B)).all()
                    if s.tol > 0.0:                                  # a warm start from a converged X: only the products in front
                        X1, infos1, _, _ = DV.dnl(L, dist, s, B, lams, JACOBI)
                        assert all(i.converged == 1 for i in infos1), (name, scheme, k)
                        n, (X2, infos2, _, _) = DV.counted(L, lambda: DV.dnl(L, dist, s, B, lams, JACOBI, X0=X1, tol=s.tol * 10))
                        assert n == per_iter and all(i.iterations == 0 for i in infos2) and M.same_bits(X2, X1).all(), (name, scheme, k, n)
    finally:
        dist.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_statuses(L):
    from libfastsparse_amd import capi
    s = DV.RECIPES0["scaled_seed0"]
    with contextlib.closing(DV.Dist(L, s, 3, False)) as dist, DV.handle_without_transpose(L, dist, s) as M_not:
        k = 3
        B, X = SV.columns(s, k), np.full((s.ncol, k), np.nan)
        bits = X.view(np.int64).copy()
        good = NL.rungs(s, k)

        def call(M_=dist.M, X_=X.ctypes.data, B_=B.ctypes.data, k_=k, lam=good, prm="default", info=None, **kw):
            f = dict(tol=1e-8, max_iter=0, precond=JACOBI, warm_start=0, diag=None)
            f.update(kw)
            p = C.byref(capi.PcgParams(f["tol"], f["max_iter"], f["precond"], f["warm_start"], f["diag"])) if prm == "default" else prm
            arr = None if lam is None else (C.c_double * len(lam))(*lam)
            return L.fs_dist_pcgn_lambdas(M_, X_, B_, k_, arr, p, info)

        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                bad = {"NULL M": call(M_=None), "NULL X": call(X_=None), "NULL B": call(B_=None), "NULL prm": call(prm=None),
                       "NULL lambda": call(lam=None), "k 0": call(k_=0), "k -1": call(k_=-1), "k too large": call(k_=N.MAX_RHS + 1, lam=[1.0] * 33),
                       "precond 3": call(precond=3), "precond -1": call(precond=-1), "DIAG without diag": call(precond=DIAG),
                       "tol < 0": call(tol=-1e-8), "tol NaN": call(tol=float("nan")), "lambda NaN": call(lam=[1.0, float("nan"), 2.0]),
                       "lambda inf": call(lam=[float("inf"), 1.0, 2.0]), "lambda -inf": call(lam=[1.0, 2.0, float("-inf")]),
                       "bad arguments on a handle without a transpose": call(M_=M_not, k_=0),
                       "a bad lambda on a handle without a transpose": call(M_=M_not, lam=[1.0, float("nan"), 2.0])}
                assert all(rc == FS_ERR_ARG for rc in bad.values()), (scheme, bad)
                assert L.fs_last_error()
                assert call(M_=M_not) == FS_ERR_NO_TRANSPOSE
                SV.refused_call_leaves(X, bits)
                infos = (capi.PcgInfo * k)()
                assert call(tol=0.0, max_iter=2, info=infos) == FS_OK    # tol = 0 is legal: the cap ends it
                assert [i.iterations for i in infos] == [2, 2, 0] and [i.converged for i in infos] == [0, 0, 1]
                assert call(lam=[-0.25, s.lam, 0.0], max_iter=3) == FS_OK    # a negative lambda is the caller's business
                X.view(np.int64)[:] = bits


def test_released_shard_of_the_transpose(L):
    """fs_matrix_release_csr on ONE rank's shard of A': Jacobi is refused before anything is written; a caller's diagonal still solves"""
    from libfastsparse_amd import capi
    s = DV.RECIPES0["scaled_seed0"]
    with G.options(binning=2, bin_flags=64):                           # kept two-pass copies: there is something to release for
        dist = DV.Dist(L, s, 3, False)
    try:
        B = SV.columns(s, 2)
        lams = NL.rungs(s, 2)
        diag = SV.caller_diag(s)
        before = {}
        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                before[scheme] = DV.dnl(L, dist, s, B, lams, DIAG, diag=diag)
                assert all(i.converged == 1 for i in DV.dnl(L, dist, s, B, lams, JACOBI)[1])
        assert L.fs_matrix_release_csr(L.fs_dist_matrix_shard(dist.M, 1, 1)) == 1
        prm = capi.PcgParams(s.tol, 0, JACOBI, 0, None)
        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                X = np.full(B.shape, np.nan)
                bits = X.view(np.int64).copy()
                assert L.fs_dist_pcgn_lambdas(dist.M, X.ctypes.data, B.ctypes.data, 2, (C.c_double * 2)(*lams), C.byref(prm), None) == FS_ERR_RELEASED
                assert b"fs_matrix_release_csr" in L.fs_last_error()
                SV.refused_call_leaves(X, bits, (scheme, "a refused solve wrote to X"))
                SV.same_solve(("a caller's diagonal after the release", scheme), DV.dnl(L, dist, s, B, lams, DIAG, diag=diag), before[scheme])
    finally:
        dist.close()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (3, 4))
def test_guard_zones(L, k):
    """X, B and diag in HBM inside guard zones, 16-byte aligned and 8 bytes off: guards untouched, inputs unchanged, and the solution
    does not depend on where the panels lie"""
    import torch
    from libfastsparse_amd import capi
    mem = LC.TorchMem()
    s = DV.RECIPES0["powerlaw_seed0"]
    F = s.ncol
    diag, B = SV.caller_diag(s), SV.columns(s, k)
    X0 = SV.x0_columns(s, B)
    lams = NL.rungs(s, k)
    arr = (C.c_double * k)(*lams)
    dist = DV.Dist(L, s, 3, False)
    try:
        gX, gB, gd = LC.Guarded(mem, "X of fs_dist_pcgn_lambdas", F * k), LC.Guarded(mem, "B of fs_dist_pcgn_lambdas", F * k), LC.Guarded(mem, "diag", F)
        for scheme in (0, 1):
            for what, precond, warm, max_iter in SV.CASES:
                ref = None
                for off in (0, 1):
                    mem.put(gB.place(F * k, off), B.reshape(-1))
                    mem.put(gd.place(F, off ^ 1), diag)
                    if warm:
                        mem.put(gX.place(F * k, off), X0.reshape(-1))
                    else:
                        mem.fill_bits(gX.place(F * k, off), LC.PREFILLS["nan"])
                    prm = capi.PcgParams(s.tol, max_iter, precond, int(warm), gd.view.data_ptr() if precond == DIAG else None)
                    infos = (capi.PcgInfo * k)()
                    with G.options(dist_cg_scheme=scheme):
                        capi.check(L.fs_dist_pcgn_lambdas(dist.M, gX.view.data_ptr(), gB.view.data_ptr(), k, arr, C.byref(prm), infos), "fs_dist_pcgn_lambdas")
                    torch.cuda.synchronize()
                    bad = mem.first_bad_guard([gX, gB, gd])
                    assert bad is None, (what, scheme, off, bad.first_broken())
                    assert mem.eq(gB.view, mem.const(B.reshape(-1))) and mem.eq(gd.view, mem.const(diag)), (what, off, "an input changed")
                    X = mem.get(gX.view)
                    assert np.isfinite(X).all(), (what, scheme, off)
                    if not max_iter and precond != NONE:
                        assert all(i.converged == 1 for i in infos), (what, scheme, off)
                    if ref is None:
                        ref = X
                    assert M.same_bits(X, ref).all(), (what, scheme, off, "the solution depends on where the panels lie")
    finally:
        dist.close()


def test_interleaved_solves_share_the_work_space_and_give_it_back(L):
    """solves of fs_dist_pcgn_lambdas (both schemes, two widths), fs_dist_pcgn, fs_dist_pcg and fs_dist_mscg interleaved on one handle
    keep their bits; after fs_dist_matrix_destroy free device memory is back where it was before the handle existed, within one
    solve's work space"""
    s = DV.RECIPES0["control_seed0"]
    B2, B5 = SV.columns(s, 2), SV.columns(s, 5)
    l2, l5 = NL.rungs(s, 2), NL.rungs(s, 5)
    ranks = 3

    def kinds(dist):
        m3 = SV.lams_of(s, "m3")
        return [DV.with_scheme(0, lambda: DV.dnl(L, dist, s, B2, l2, JACOBI)[0]), DV.with_scheme(1, lambda: DV.dnl(L, dist, s, B2, l2, JACOBI)[0]),
                lambda: DV.dpcgn(L, dist, s, B2, JACOBI)[0], DV.with_scheme(1, lambda: DV.dnl(L, dist, s, B5, l5, DIAG, diag=SV.caller_diag(s), hbm=True)[0]),
                DV.with_scheme(1, lambda: DV.dpcg(L, dist, s, JACOBI)[0]), DV.with_scheme(0, lambda: DV.dnl(L, dist, s, B5, l5, JACOBI, X0=SV.x0_columns(s, B5))[0]),
                DV.with_scheme(1, lambda: DV.dmscg(L, dist, s, m3)[0]), lambda: DV.dpcgn(L, dist, s, B5, JACOBI)[0],
                DV.with_scheme(0, lambda: DV.dpcg(L, dist, s, JACOBI)[0]), DV.with_scheme(1, lambda: DV.dnl(L, dist, s, B5, l5, NONE, max_iter=7)[0])]

    k = 5
    one_solve = 8 * (3 * k * s.ncol + k * s.nrow + s.ncol + 2048 * k + 512)      # the allowance of test_gpu_dist_pcg.py's
    DV.interleaved_then_memory_back(L, s, ranks, kinds, 6, one_solve)


# ---- 10 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,ranks", [("coo", 3), ("cuts", 3), ("cuts", 5)])
def test_pair_handle(L, route, ranks):
    """fs_dist_matrix_pair(A, At): A' in the caller's entry order, cut where the caller cut it: both schemes are the models on that A'
    and those bounds"""
    for name in DPair.RECIPES0[1:] + ("binary_F65", "valued", "lambda0_empty_column"):
        s = DV.PAIR_SYSTEMS[name]
        pd = DV.PairDist(L, s, ranks, route)
        try:
            bounds = pd.bounds_t()
            t = pd.t_csr()
            for k, case in ((3, 1), (8, 6), (2, 0)):
                B = SV.columns(s, k)
                lams = NL.rungs(s, k)
                what, precond, X0, max_iter, diag = _case(s, B, case, t)
                for scheme in (0, 1):
                    with G.options(strict_order=1, dist_cg_scheme=scheme):
                        got = DV.dnl(L, pd, s, B, lams, precond, X0, max_iter, diag, hbm=scheme == 1)
                    entry = f"fs_dist_pcgn_lambdas scheme {scheme} k {k} {what} on a pair, route {route}, bounds {bounds}, on {name}"
                    DV.assert_dnl_model(entry, got, _model(s, B, lams, precond, X0, max_iter, diag, t, bounds if scheme == 1 else None))
        finally:
            pd.close()
