"""fs_dist_mscg on virtual ranks of one device (fs_dist_create(n, [0] * n)), against the CPU models (tests/_mscg_model.py,
_dist_mscg_model.py) and against the single-device and the other sharded solvers, on the harness of tests/_solvers.py and
tests/_dist_solvers.py.  A' of every model is dist.t_csr(): the shards' own rows, downloaded.

1  strict_order, scheme 0: X, the infos, st[] and the per-shift array are the whole-tree model's on 1 and 3 ranks, A' built on the
   host and on the device, ladders m1 / m3 / m8 (shuffled), uncapped and under a cap of 5, X in host memory and in HBM, packed and
   padded; on three ranks also a single-device fs_mscg on the same CSRs.  binary_F262145 once, m3 under a cap of 5.
2  strict_order, scheme 1 on three ranks: the slice model on bounds_t(); the recipes are first shown, on the CPU, to tell the two
   schemes apart; five ranks on three unknowns leave empty slices; binary_F262145 once.
3  shifts {lam, lam + 1e6, lam + 1e9} at tol 1e-14 on slices: finite, converged, the slice model's bits (a frozen shift's slice is
   never written again).
4  m = 1 is fs_dist_pcg without a preconditioner from a cold start, both schemes, every mode.
5  the columns of the smallest lambda, duplicates included, are fs_dist_cg's x and count, both schemes, every mode.
6  default mode, the ladder of eight on the recipes, both schemes: converged, true residual <= 2 tol, solves repeat their bits.
7  the number of sharded products per solve; none for a solve that is done at its start.
8  statuses, with X untouched by every refused call; a product's own error is passed through.
9  guard zones, interleaved solves on one handle, device memory given back.
10 a pair handle: the caller's entry order of A' and the caller's cuts."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import _cg_model as M
import _dist_pair as DPair
import _dist_solvers as DV
import _gpu as G
import _lifecycle as LC
import _mscg_model as S
import _pcg_model as P
import _solvers as SV
from _gpu import FS_ERR_ARG, FS_ERR_NO_TRANSPOSE, FS_ERR_RELEASED, FS_OK, L  # noqa: F401

pytestmark = pytest.mark.gpu

SMALL = [n for n in DV.MSCG_ALL if n != "binary_F262145"]                    # (the models are Python: the large system runs once per scheme)
LADDERS = {k: SV.LADDERS[k] for k in ("m1", "m3", "m8")}


def _assert_same_solve(what, got, want):
    """two device solves: X, the infos and the per-shift array, bit for bit"""
    assert M.same_bits(got[0], want[0]).all(), what
    SV.assert_infos(what, got[1], [S.Info(i.iterations, i.converged, i.rnorm, i.bnorm) for i in want[1]])
    bad = S.shifts_mismatch(got[3], want[3])
    assert bad is None, (what, bad)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_scheme0_strict_is_fs_mscg(L, name):
    s = DV.MSCG_ALL[name]
    F = s.ncol
    single = {}
    n = 0
    for ranks, device_t in ((1, False), (3, False), (3, True), (1, True)):
        dist = DV.Dist(L, s, ranks, device_t)
        try:
            t_csr = DV.sorted_t(dist, s)
            with G.options(strict_order=1, dist_cg_scheme=0):
                for ladder in LADDERS:
                    for cap in (0, 5):
                        n += 1
                        hbm, ldx = n % 2 == 1, F + 3 * (n // 2 % 2)
                        lams = SV.lams_of(s, ladder)
                        got = DV.dmscg(L, dist, s, lams, cap, hbm=hbm, ldx=ldx)
                        what = (f"fs_dist_mscg scheme 0 {ladder} cap {cap}, {ranks} ranks, {'device' if device_t else 'host'} A', "
                                f"{'HBM' if hbm else 'host'} vectors, ldx {ldx}, on {name}")
                        DV.assert_dmscg_model(what, got, DV.dmscg_model(s, ladder, cap, t_csr))
                        if ranks == 3 and not device_t:              # a single-device fs_mscg on the same CSRs
                            if not single:
                                single["h"] = SV.single_handles(L, s)
                            _assert_same_solve(what + " vs fs_mscg", got, SV.mscg_run(L, single["h"][0], single["h"][1], s, lams, cap, ldx=ldx))
                        if name == "zero_rhs":
                            assert all(i.converged == 1 and i.iterations == 0 for i in got[1]) and M.same_bits(got[0], np.zeros(got[0].shape)).all()
        finally:
            dist.close()


def test_scheme0_more_than_one_grid_stride_capped(L):
    s = DV.MSCG_ALL["binary_F262145"]
    lams = SV.lams_of(s, "m3")
    single = SV.single_handles(L, s)
    dist = DV.Dist(L, s, 3, False)
    try:
        t_csr = DV.sorted_t(dist, s)
        with G.options(strict_order=1, dist_cg_scheme=0):
            got = DV.dmscg(L, dist, s, lams, 5, hbm=True, ldx=s.ncol + 3)
            DV.assert_dmscg_model("fs_dist_mscg scheme 0 m3 cap 5 on binary_F262145", got, DV.dmscg_model(s, "m3", 5, t_csr))
            _assert_same_solve("binary_F262145 vs fs_mscg", got, SV.mscg_run(L, single[0], single[1], s, lams, 5))
        assert [i.iterations for i in got[1]] == [5, 5, 5] and not any(i.converged for i in got[1])
    finally:
        dist.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_scheme1_strict_is_the_slice_model(L, name):
    s = DV.MSCG_ALL[name]
    F = s.ncol
    n = 0
    for device_t in (False, True):
        dist = DV.Dist(L, s, 3, device_t)
        try:
            bounds = dist.bounds_t()
            assert bounds[0] == 0 and bounds[-1] == F
            t_csr = DV.sorted_t(dist, s)
            if name in DV.MSCG_RECIPES0:                                     # on the CPU first: the slice tree is told from the whole one
                whole, sliced = DV.dmscg_model(s, "m8", 0, t_csr), DV.dmscg_model(s, "m8", 0, t_csr, bounds)
                differ = [int((~M.same_bits(whole.X[i], sliced.X[i])).sum()) for i in range(len(whole.infos))]
                print(f"{name} bounds {bounds}: entries of {F} that differ between the slice model and the whole model, per shift: {differ}")
                # (these are the handle's own cuts, not _dist_mscg_model.DIFFERING_BOUNDS: a shift large enough to converge in its
                # first iterations may keep its bits, the ladder as a whole must not)
                assert all(a < b for a, b in zip(bounds, bounds[1:])) and sum(d >= 1 for d in differ) >= len(differ) // 2, (name, bounds, differ)
            with G.options(strict_order=1, dist_cg_scheme=1):
                for ladder in LADDERS:
                    for cap in (0, 5):
                        n += 1
                        hbm, ldx = n % 2 == 0, F + 3 * (n // 2 % 2)
                        got = DV.dmscg(L, dist, s, SV.lams_of(s, ladder), cap, hbm=hbm, ldx=ldx)
                        what = f"fs_dist_mscg scheme 1 {ladder} cap {cap}, bounds {bounds}, {'HBM' if hbm else 'host'} vectors, ldx {ldx}, on {name}"
                        DV.assert_dmscg_model(what, got, DV.dmscg_model(s, ladder, cap, t_csr, bounds))
        finally:
            dist.close()


def test_scheme1_with_empty_slices(L):
    """five ranks on the three rows of A': some slices are empty and contribute +0.0"""
    s = DV.MSCG_ALL["three_eigenvalues"]
    dist = DV.Dist(L, s, 5, False)
    try:
        bounds = dist.bounds_t()
        assert any(a == b for a, b in zip(bounds, bounds[1:])), bounds
        t_csr = DV.sorted_t(dist, s)
        with G.options(strict_order=1, dist_cg_scheme=1):
            for ladder in LADDERS:
                for cap in (0, 2):
                    got = DV.dmscg(L, dist, s, SV.lams_of(s, ladder), cap, hbm=cap == 2)
                    DV.assert_dmscg_model(f"fs_dist_mscg scheme 1 {ladder} cap {cap}, bounds {bounds}", got, DV.dmscg_model(s, ladder, cap, t_csr, bounds))
    finally:
        dist.close()


def test_scheme1_more_than_one_grid_stride_capped(L):
    s = DV.MSCG_ALL["binary_F262145"]
    dist = DV.Dist(L, s, 3, True)
    try:
        bounds = dist.bounds_t()
        t_csr = DV.sorted_t(dist, s)
        with G.options(strict_order=1, dist_cg_scheme=1):
            got = DV.dmscg(L, dist, s, SV.lams_of(s, "m3"), 5, ldx=s.ncol + 3)
        DV.assert_dmscg_model(f"fs_dist_mscg scheme 1 m3 cap 5 on binary_F262145, bounds {bounds}", got, DV.dmscg_model(s, "m3", 5, t_csr, bounds))
    finally:
        dist.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DV.MSCG_RECIPES0))
def test_large_shifts_freeze_on_slices(L, name):
    s = DV.MSCG_RECIPES0[name]
    lams = [s.lam, s.lam + 1e6, s.lam + 1e9]
    dist = DV.Dist(L, s, 3, False)
    try:
        bounds = dist.bounds_t()
        t_csr = DV.sorted_t(dist, s)
        with G.options(strict_order=1, dist_cg_scheme=1):
            got = DV.dmscg(L, dist, s, lams, tol=1e-14, hbm=True)
        X, infos, st, shifts = got
        print(f"{name}: counts {[i.iterations for i in infos]}, rnorm {[i.rnorm for i in infos]}")
        assert np.isfinite(X).all() and all(np.isfinite(v).all() for v in shifts.values()), name
        assert all(i.converged == 1 for i in infos), (name, [(i.iterations, i.converged) for i in infos])
        DV.assert_dmscg_model(f"fs_dist_mscg scheme 1 large shifts on {name}", got, DV.dmscg_model(s, "large", 0, t_csr, bounds, lams=lams, tol=1e-14))
    finally:
        dist.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_one_lambda_is_fs_dist_pcg_without_preconditioner(L, mode):
    for name in SMALL:
        s = DV.MSCG_ALL[name]
        dist = DV.Dist(L, s, 3, False)
        try:
            for scheme in (0, 1):
                for cap in (0, 5):
                    with G.mode_options(mode), G.options(dist_cg_scheme=scheme):
                        xp, ip, stp = DV.dpcg(L, dist, s, max_iter=cap)
                        X, infos, st, _ = DV.dmscg(L, dist, s, [s.lam], cap)
                    want = dict(stp)
                    if ip.converged == 1 and ip.iterations == 0 and M.same_bits(xp, np.zeros(s.ncol)).all():
                        for k in ("rsq", "alpha", "beta"):           # done before the first iteration: fs_pcg never writes these
                            want.pop(k)
                    elif ip.iterations == 0:
                        want.pop("beta")                             # (never written by either)
                    what = (name, mode, scheme, cap)
                    bad = M.mismatch(X[0], xp, infos[0].iterations, ip.iterations, st, want)
                    assert bad is None, (what, bad)
                    SV.assert_infos(what, infos, [S.Info(ip.iterations, ip.converged, ip.rnorm, ip.bnorm)])
        finally:
            dist.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_columns_of_the_smallest_lambda_are_fs_dist_cg(L, mode):
    for name in SMALL:
        s = DV.MSCG_ALL[name]
        if not np.any(s.b != 0):
            continue
        dist = DV.Dist(L, s, 3, False)
        try:
            for scheme in (0, 1):
                with G.mode_options(mode), G.options(dist_cg_scheme=scheme):
                    xc, itc, stc = dist.cg(False)
                    for ladder in ("m3", "m8"):
                        lams = SV.lams_of(s, ladder)
                        X, infos, st, shifts = DV.dmscg(L, dist, s, lams)
                        cols = [i for i, lam in enumerate(lams) if lam == min(lams)]
                        assert min(lams) == s.lam and len(cols) == {"m3": 2, "m8": 1}[ladder]
                        for i in cols:
                            what = (name, mode, scheme, ladder, i)
                            assert M.same_bits(X[i], xc).all() and infos[i].iterations == itc, (what, M.mismatch(X[i], xc, infos[i].iterations, itc))
                            assert infos[i].converged == int(stc["done"]) and shifts["z"][i] == 1.0 and shifts["pslot"][i] == -1.0, what
        finally:
            dist.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def assert_default_mode_bars(L, dist, s):
    """the ladder of eight in the default mode, both schemes, on any handle with a transposed side"""
    lams = [s.lam * f for f in S.LADDER]
    for scheme in (0, 1):
        with G.options(dist_cg_scheme=scheme):
            runs = [DV.dmscg(L, dist, s, lams, hbm=scheme == 1) for _ in range(2)]
        X, infos, _, _ = runs[0]
        res = [SV.residual(s, X[i], lam) for i, lam in enumerate(lams)]
        print(f"{s.name} scheme {scheme}: counts {[i.iterations for i in infos]}, true residuals / tol {[round(r / s.tol, 2) for r in res]}")
        for i, lam in enumerate(lams):
            what = (s.name, scheme, i, lam, infos[i].iterations, res[i])
            assert infos[i].converged == 1, what
            assert res[i] <= 2 * s.tol, what
            assert infos[i].rnorm <= s.tol * infos[i].bnorm, what
        assert M.same_bits(runs[1][0], X).all() and [i.iterations for i in runs[1][1]] == [i.iterations for i in infos], (s.name, scheme)


@pytest.mark.parametrize("name", list(DV.MSCG_RECIPES0))
def test_default_mode_ladder_within_the_bars(L, name):
    s = DV.MSCG_RECIPES0[name]
    dist = DV.Dist(L, s, 3, False)
    try:
        assert_default_mode_bars(L, dist, s)
    finally:
        dist.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
PRODUCT_SET = ("three_eigenvalues", "cap_tol0", "fixture_100x50") + tuple(DV.MSCG_RECIPES0)


@pytest.mark.parametrize("name", PRODUCT_SET)
def test_sharded_products_per_solve(L, name):
    """fs_debug_dist_products() per solve, strict mode, three ranks: per_iter x min(cap, st[iter] + 2) with per_iter = 2 sharded products
    (replicate) or 1 (slices: A' is the rank's own shard); none for a solve that is done at its start"""
    s = DV.MSCG_ALL[name]
    F = s.ncol
    dist = DV.Dist(L, s, 3, False)
    try:
        for scheme, per_iter in ((0, 2), (1, 1)):
            with G.options(strict_order=1, dist_cg_scheme=scheme):
                for ladder in ("m1", "m8"):
                    for max_iter in (0, 2):
                        n, (X, infos, st, _) = DV.counted(L, lambda: DV.dmscg(L, dist, s, SV.lams_of(s, ladder), max_iter))
                        at_start = st["done"] == 1.0 and st["iter"] == 0.0 and bool(M.same_bits(X, np.zeros(X.shape)).all())
                        what = (name, scheme, ladder, max_iter, n, st["iter"], st["done"], at_start)
                        print(*what)
                        assert n == per_iter * DV.loops(max_iter or F, int(st["iter"]), at_start), what
                for tol, b in ((s.tol, np.zeros(F)), (1.0, s.b), (2.5, s.b)):        # done at the start: b = 0, tol >= 1
                    n, (X, infos, st, _) = DV.counted(L, lambda: DV.dmscg(L, dist, s, SV.lams_of(s, "m3"), tol=tol, b=b))
                    assert n == 0, (name, scheme, tol, n)
                    assert all(i.converged == 1 and i.iterations == 0 for i in infos) and M.same_bits(X, np.zeros(X.shape)).all(), (name, scheme, tol)
    finally:
        dist.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_statuses(L):
    from libfastsparse_amd import capi
    s = DV.MSCG_RECIPES0["control_seed0"]
    with contextlib.closing(DV.Dist(L, s, 3, False)) as dist, DV.handle_without_transpose(L, dist, s) as M_not:
        F, m = s.ncol, 3
        b, X = s.b.copy(), np.full(16 * F, np.nan)
        bits = X.view(np.int64).copy()
        lams = [s.lam * 3, s.lam, s.lam * 10]

        def call(M_=dist.M, X_=X.ctypes.data, ldx=F, b_=b.ctypes.data, m_=m, lam="default", tol=1e-8, max_iter=0, info=None):
            if lam == "default":
                lam = lams + [1.0] * (max(m_, m) - m)
            arr = None if lam is None else (C.c_double * len(lam))(*lam)
            return L.fs_dist_mscg(M_, X_, ldx, b_, m_, arr, tol, max_iter, info)

        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                bad = {"NULL M": call(M_=None), "NULL X": call(X_=None), "NULL b": call(b_=None), "NULL lambda": call(lam=None),
                       "m 0": call(m_=0), "m -1": call(m_=-1), "m 17": call(m_=17), "ldx < F": call(ldx=F - 1), "ldx 0": call(ldx=0),
                       "tol < 0": call(tol=-1e-8), "tol NaN": call(tol=float("nan")), "tol -inf": call(tol=float("-inf")),
                       "lambda NaN": call(lam=[1.0, float("nan"), 2.0]), "lambda inf": call(lam=[float("inf"), 1.0, 2.0]),
                       "lambda -inf": call(lam=[1.0, 2.0, float("-inf")]),
                       "bad arguments on a handle without a transpose": call(M_=M_not, m_=0)}
                assert all(rc == FS_ERR_ARG for rc in bad.values()), (scheme, bad)
                assert L.fs_last_error()
                assert call(M_=M_not) == FS_ERR_NO_TRANSPOSE
                SV.refused_call_leaves(X, bits)
                assert call(tol=0.0, max_iter=2) == FS_OK            # tol = 0 is legal: the cap ends it (info NULL is legal too)
                assert call(m_=16) == FS_OK
                infos = (capi.PcgInfo * m)()
                assert call(tol=0.0, max_iter=2, info=infos) == FS_OK
                assert [i.iterations for i in infos] == [2, 2, 2] and not any(i.converged for i in infos)
                assert call(lam=[-0.25, s.lam, 0.0], max_iter=3) == FS_OK   # a negative lambda is the caller's business
                X.view(np.int64)[:] = bits


def test_a_product_error_is_passed_through(L):
    """fs_matrix_release_csr on ONE rank's shard of A': under strict_order a product reads the plain CSR, so the solve ends with
    FS_ERR_RELEASED and the product's message, X untouched; outside strict_order the kept copy serves and the solve is the one from
    before the release"""
    s = SV.RECIPES["scaled_seed0"]                                    # (the system test_gpu_dist_pcg.py releases a shard of; plain CG
    lams = SV.lams_of(s, "m3")                                          # does not converge on it: the solves run under a cap)
    arr = (C.c_double * len(lams))(*lams)
    with G.options(binning=2, bin_flags=64):                           # kept two-pass copies: there is something to release for
        dist = DV.Dist(L, s, 3, False)
    try:
        before = {}
        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                before[scheme] = DV.dmscg(L, dist, s, lams, 20)
                assert np.isfinite(before[scheme][0]).all()
        assert L.fs_matrix_release_csr(L.fs_dist_matrix_shard(dist.M, 1, 1)) == 1
        for scheme in (0, 1):
            X = np.full(len(lams) * s.ncol, np.nan)
            bits = X.view(np.int64).copy()
            with G.options(strict_order=1, dist_cg_scheme=scheme):
                assert L.fs_dist_mscg(dist.M, X.ctypes.data, s.ncol, s.b.ctypes.data, len(lams), arr, s.tol, 20, None) == FS_ERR_RELEASED, scheme
                assert b"fs_matrix_release_csr" in L.fs_last_error()
            SV.refused_call_leaves(X, bits, (scheme, "a refused solve wrote to X"))
            with G.options(dist_cg_scheme=scheme):
                after = DV.dmscg(L, dist, s, lams, 20)                  # the kept copy needs no plain array
            _assert_same_solve(("after the release", scheme), after, before[scheme])
    finally:
        dist.close()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DV.MSCG_RECIPES0))
def test_guard_zones(L, name):
    """X (packed and padded) and b in HBM inside guard zones, 16-byte aligned and 8 bytes off: guards untouched, b unchanged, the gaps
    between the x_i keep their bits, and the solution does not depend on where X lies"""
    import torch
    from libfastsparse_amd import capi
    mem = LC.TorchMem()
    s = DV.MSCG_RECIPES0[name]
    F = s.ncol
    dist = DV.Dist(L, s, 3, False)
    try:
        gx, gb = LC.Guarded(mem, "X of fs_dist_mscg", 8 * (F + 3)), LC.Guarded(mem, "b of fs_dist_mscg", F)
        for scheme in (0, 1):
            for ladder, cap in (("m1", 0), ("m3", 0), ("m8", 0), ("m8", 5)):
                lams = SV.lams_of(s, ladder)
                m = len(lams)
                ref = None
                for ldx in (F, F + 3):
                    for off in (0, 1):
                        mem.put(gb.place(F, off ^ (ldx & 1)), s.b)
                        n = (m - 1) * ldx + F
                        mem.fill_bits(gx.place(n, off), SV.GAP_BITS)
                        infos = (capi.PcgInfo * m)()
                        with G.options(dist_cg_scheme=scheme):
                            capi.check(L.fs_dist_mscg(dist.M, gx.view.data_ptr(), ldx, gb.view.data_ptr(), m, (C.c_double * m)(*lams), s.tol, cap,
                                                      infos), "fs_dist_mscg")
                        torch.cuda.synchronize()
                        what = (name, scheme, ladder, cap, ldx, off)
                        bad = mem.first_bad_guard([gx, gb])
                        assert bad is None, (what, bad.first_broken())
                        assert mem.eq(gb.view, mem.const(s.b)), (what, "b changed")
                        X, gaps = SV.split_rows_and_gaps(mem.get(gx.view), m, F, ldx)
                        assert (gaps.view(np.int64) == SV.GAP_BITS).all(), (what, "a gap between the x_i was written")
                        assert np.isfinite(X).all(), what
                        if not cap:
                            assert all(i.converged == 1 for i in infos), (what, [i.iterations for i in infos])
                        if ref is None:
                            ref = X
                        assert M.same_bits(X, ref).all(), (what, "the solution depends on where X lies")
    finally:
        dist.close()


def test_interleaved_solves_share_the_work_space_and_give_it_back(L):
    """solves of fs_dist_cg, fs_dist_pcg, fs_dist_pcgn and fs_dist_mscg (m3, then m8: the work space grows; both schemes) interleaved
    on one handle keep their bits; after fs_dist_matrix_destroy free device memory is back where it was before the handle existed,
    within one solve's work space"""
    s = DV.MSCG_RECIPES0["control_seed0"]
    B2 = SV.columns(s, 2)
    ranks = 3

    def kinds(dist):
        m3, m8 = SV.lams_of(s, "m3"), SV.lams_of(s, "m8")
        return [DV.with_scheme(0, lambda: dist.cg(False)[0]), DV.with_scheme(0, lambda: DV.dmscg(L, dist, s, m3)[0]),
                DV.with_scheme(1, lambda: DV.dpcg(L, dist, s, P.PRECOND_JACOBI)[0]), DV.with_scheme(1, lambda: DV.dmscg(L, dist, s, m3, hbm=True)[0]),
                lambda: DV.dpcgn(L, dist, s, B2, P.PRECOND_JACOBI)[0], DV.with_scheme(0, lambda: DV.dmscg(L, dist, s, m8, ldx=s.ncol + 3)[0]),
                DV.with_scheme(1, lambda: dist.cg(False)[0]), DV.with_scheme(1, lambda: DV.dmscg(L, dist, s, m8)[0]),
                DV.with_scheme(0, lambda: DV.dpcg(L, dist, s, P.PRECOND_JACOBI)[0]), DV.with_scheme(1, lambda: DV.dmscg(L, dist, s, m3, max_iter=5)[0])]

    # one solve's work space, the larger scheme (replicate): per rank the m x_i and the nslots P_i of the m8 ladder, F doubles each
    # rounded up to even, and the per-shift array
    m, nslots = 8, 7
    one_solve = 8 * ranks * ((m + nslots) * (s.ncol + 1) + S.MAX_SHIFTS * S.MS_STRIDE)
    DV.interleaved_then_memory_back(L, s, ranks, kinds, 5, one_solve)


# ---- 10 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,ranks", [("coo", 3), ("cuts", 3), ("cuts", 5)])
def test_pair_handle(L, route, ranks):
    """fs_dist_matrix_pair(A, At): A' in the caller's entry order, cut where the caller cut it (an empty slice in front and a one-row
    slice with the caller's cuts on three ranks, empty slices in the middle on five): both schemes are the models on that A' and those
    bounds"""
    for name in DPair.RECIPES0[1:] + ("binary_F65", "valued", "lambda0_empty_column"):
        s = DV.PAIR_SYSTEMS[name]
        pd = DV.PairDist(L, s, ranks, route)
        try:
            bounds = pd.bounds_t()
            t = pd.t_csr()
            for scheme in (0, 1):
                with G.options(strict_order=1, dist_cg_scheme=scheme):
                    for ladder, cap in (("m3", 0), ("m8", 0), ("m8", 5)):
                        got = DV.dmscg(L, pd, s, SV.lams_of(s, ladder), cap, hbm=cap == 5, ldx=s.ncol + 3 * scheme)
                        what = f"fs_dist_mscg scheme {scheme} {ladder} cap {cap} on a pair, route {route}, bounds {bounds}, on {name}"
                        DV.assert_dmscg_model(what, got, DV.dmscg_model(s, ladder, cap, t, bounds if scheme == 1 else None))
        finally:
            pd.close()
