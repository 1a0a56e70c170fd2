"""fs_dist_mscgn on virtual ranks of one device (fs_dist_create(n, [0] * n)), against the CPU model (tests/_dist_mscgn_model.py: column
j is the model of fs_dist_mscg on B[:, j]), against fs_mscgn on one device and against the other sharded solvers, on the harness of
tests/_solvers.py and tests/_dist_solvers.py.  A' of every model is dist.t_csr(): the shards' own rows, downloaded.

1  strict_order, scheme 0, on 1 and 3 ranks, A' built on the host and on the device: the whole model's bits (X, infos, rank 0's
   per-column st[] / ms[]) and those of a single-device fs_mscgn on the same CSRs -- k in (1, 2, 3, 4, 5, 8, 17, 32) (the step kernel
   takes 16 columns per pass), ladders m1 / m3 / m8 (shuffled) / m16, caps 0 and 5, both forms of the kernels for k > 4, X in host
   memory and in HBM, ldx = F k and F k + 3 with the gaps' bits asserted.
2  strict_order, scheme 1 on three ranks: the slice model on bounds_t(), which is first shown, on the CPU, to differ from the whole
   model in at least half of the non-zero columns; odd k on slices of odd length; five ranks on three unknowns leave empty slices.
3  F = 262145 on three ranks (more than one grid stride per whole panel, slices of 87 381 rows), cap 3, both schemes, k = 2, m3.
4  identities, in every mode in which the right-hand solver repeats its bits: m = 1 is fs_dist_pcgn_lambdas with equal lambdas and no
   preconditioner (scheme 1) and fs_dist_pcgn (scheme 0); k = 1 is fs_dist_mscg (both schemes); the pairs of the smallest lambda have
   fs_dist_cg's x and count on their column.
5  shifts {lam, lam + 1e6, lam + 1e9} at tol 1e-14 on slices: finite, converged, the slice model's bits, a shift without a live pair
   is not written again; a NaN in one column of B stays in its column.
6  default mode, the ladder of eight, k = 4, both recipes, both schemes: converged, true residual <= 2 tol ||b_j||, solves repeat.
7  sharded products per solve: 2 per iteration under scheme 0, 1 under scheme 1, none for a solve done at its start.
8  statuses, with X untouched by every refused call; a product's own error is passed through.
9  guard zones, interleaved solves on one handle, device memory given back.
10 a pair handle: both schemes are the models on the caller's A' order and the caller's cuts (DIFFERING_BOUNDS)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import _cg_model as M
import _dist_mscgn_model as DN
import _dist_solvers as DV
import _gpu as G
import _lifecycle as LC
import _mscg_model as S
import _pcg_model as P
import _pcgn_model as N
import _solvers as SV
from _gpu import FS_ERR_ARG, FS_ERR_NO_TRANSPOSE, FS_ERR_RELEASED, FS_OK, L  # noqa: F401

pytestmark = pytest.mark.gpu

COMBOS = [(ladder, cap) for ladder in ("m1", "m3", "m8", "m16") for cap in (0, 5)]
_CACHE = {}


def test_the_cases_cover_what_they_should():
    assert DV.KS == (1, 2, 3, 4, 5, 8, 17, 32) and set(SV.LADDERS) == {"m1", "m3", "m8", "m16"}
    assert {len(SV.LADDERS[l]) for l in SV.LADDERS} == {1, 3, 8, 16} and SV.LADDERS["m3"].count(min(SV.LADDERS["m3"])) == 2
    assert tuple(sorted(SV.LADDERS["m8"])) == tuple(sorted(S.LADDER)) and SV.LADDERS["m8"] != tuple(S.LADDER)          # shuffled
    seen = {c for i in range(len(DV.KS)) for c in _combos(i)}
    assert seen == set(COMBOS)                                        # every ladder under both caps, over the ks
    assert M.RED_THREADS // S.MAX_SHIFTS == 16 and any(k > 16 for k in DV.KS) and 17 in DV.KS     # the step kernel's columns per pass


def _combos(i):
    """the two (ladder, cap) of the i-th k: over the eight ks every ladder meets both caps"""
    return COMBOS[i % 8], COMBOS[(i + 5) % 8]


def _model(s, B, lams, cap, t_csr, bounds=None, tol=None):
    return DN.run(s, B, lams, max_iter=cap, tol=tol, t_csr=t_csr, bounds=bounds, cache=_CACHE)


_assert_model = DV.assert_dmscgn_model


def _assert_same_solve(what, got, want):
    """two device solves: X, the infos and every column's state and per-shift array, bit for bit (want: dmscgn's or mscgn_run's)"""
    assert M.same_bits(got[0], want[0]).all(), (what, int((~M.same_bits(got[0], want[0])).sum()))
    for j in range(got[0].shape[2]):
        SV.assert_infos((what, j), [row[j] for row in got[1]], [S.Info(r[j].iterations, r[j].converged, r[j].rnorm, r[j].bnorm) for r in want[1]])
        bad = M.mismatch(np.zeros(0), np.zeros(0), None, None, got[2][j][0], want[2][j][0]) or S.shifts_mismatch(got[2][j][1], want[2][j][1])
        assert bad is None, (what, j, bad)


def _kernels(k):
    return (1, 2) if k > 4 else (0,)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", DV.KS)
def test_scheme0_strict_is_fs_mscgn_and_the_model(L, k):
    s, B = DV.panel(k)
    ne = s.ncol * k
    single = SV.single_handles(L, s)
    n = 0
    for ranks, device_t in ((1, False), (3, True), (3, False)):
        dist = DV.Dist(L, s, ranks, device_t)
        try:
            t_csr = DV.sorted_t(dist, s)
            for ladder, cap in _combos(DV.KS.index(k)):
                lams = SV.lams_of(s, ladder)
                model = _model(s, B, lams, cap, t_csr)
                for kernel in _kernels(k):
                    n += 1
                    hbm, ldx = n % 2 == 1, ne + 3 * (n // 2 % 2)
                    with G.options(strict_order=1, pcgn_kernel=kernel, dist_cg_scheme=0):
                        got = DV.dmscgn(L, dist, s, B, lams, cap, hbm=hbm, ldx=ldx)
                        one = SV.mscgn_run(L, single[0], single[1], s, B, lams, cap)
                    what = (f"fs_dist_mscgn scheme 0 k {k} {ladder} cap {cap}, {ranks} ranks, {'device' if device_t else 'host'} A', "
                            f"pcgn_kernel {kernel}, {'HBM' if hbm else 'host'} panels, ldx {ldx}")
                    _assert_model(what, got, model)
                    _assert_same_solve(what + " vs fs_mscgn", got, one)
                    if cap:
                        assert all(i.iterations <= cap for row in got[1] for i in row), what
        finally:
            dist.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", DV.KS)
def test_scheme1_strict_is_the_slice_model(L, k):
    s, B = DV.panel(k)
    ne = s.ncol * k
    n = 0
    for device_t in (False, True):
        dist = DV.Dist(L, s, 3, device_t)
        try:
            bounds = dist.bounds_t()
            assert bounds[0] == 0 and bounds[-1] == s.ncol and all(a < b for a, b in zip(bounds, bounds[1:]))
            t_csr = DV.sorted_t(dist, s)
            for ladder, cap in _combos(DV.KS.index(k)):
                lams = SV.lams_of(s, ladder)
                whole, sliced = _model(s, B, lams, cap, t_csr), _model(s, B, lams, cap, t_csr, bounds)
                nz = SV.nonzero_columns(B)                             # on the CPU first: the slice tree is told from the whole one
                differ = DN.differing_columns(sliced, whole)
                print(f"k {k} {ladder} cap {cap} bounds {bounds}: {len(differ)} of {len(nz)} non-zero columns differ between the slice model and the whole model")
                assert set(differ) <= set(nz) and 2 * len(differ) >= len(nz), (k, ladder, cap, bounds, differ)
                for kernel in _kernels(k):
                    n += 1
                    hbm, ldx = n % 2 == 0, ne + 3
                    with G.options(strict_order=1, pcgn_kernel=kernel, dist_cg_scheme=1):
                        got = DV.dmscgn(L, dist, s, B, lams, cap, hbm=hbm, ldx=ldx)
                    _assert_model(f"fs_dist_mscgn scheme 1 k {k} {ladder} cap {cap}, bounds {bounds}, pcgn_kernel {kernel}, "
                                  f"{'HBM' if hbm else 'host'} panels, ldx {ldx}", got, sliced)
        finally:
            dist.close()


@pytest.mark.parametrize("k", (3, 5, 17))
def test_scheme1_odd_k_on_slices_of_odd_length(L, k):
    """ne = rows k is odd on a slice: the flat pair kernels take a slice as a panel of fewer rows, 8 bytes at a time"""
    s = DV.ALL["binary_F65"]
    B = SV.columns(s, k)
    dist = DV.Dist(L, s, 3, False)
    try:
        bounds = dist.bounds_t()
        rows = [b - a for a, b in zip(bounds, bounds[1:])]
        assert sum(r % 2 for r in rows) >= 1 and all((r * k) % 2 == r % 2 for r in rows), rows
        t_csr = DV.sorted_t(dist, s)
        for ladder, cap in (("m3", 0), ("m8", 5)):
            lams = SV.lams_of(s, ladder)
            for kernel in _kernels(k):
                with G.options(strict_order=1, pcgn_kernel=kernel, dist_cg_scheme=1):
                    got = DV.dmscgn(L, dist, s, B, lams, cap, hbm=cap == 5, ldx=s.ncol * k + 3)
                _assert_model(f"fs_dist_mscgn scheme 1 k {k} {ladder} cap {cap}, slices of {rows} rows", got, _model(s, B, lams, cap, t_csr, bounds))
    finally:
        dist.close()


def test_scheme1_with_empty_slices(L):
    """five ranks on the three rows of A': some slices are empty and contribute +0.0"""
    s = DV.ALL["three_eigenvalues"]
    dist = DV.Dist(L, s, 5, False)
    try:
        bounds = dist.bounds_t()
        assert len(bounds) == 6 and any(a == b for a, b in zip(bounds, bounds[1:])), bounds
        t_csr = DV.sorted_t(dist, s)
        for k in (1, 3, 8):
            B = SV.columns(s, k)
            for ladder, cap in (("m3", 0), ("m8", 2)):
                lams = SV.lams_of(s, ladder)
                for kernel in _kernels(k):
                    with G.options(strict_order=1, pcgn_kernel=kernel, dist_cg_scheme=1):
                        got = DV.dmscgn(L, dist, s, B, lams, cap, hbm=cap == 2, ldx=s.ncol * k + 3)
                    _assert_model(f"fs_dist_mscgn scheme 1 k {k} {ladder} cap {cap}, bounds {bounds}", got, _model(s, B, lams, cap, t_csr, bounds))
    finally:
        dist.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_large_panels_capped(L):
    s = DV.ALL["binary_F262145"]
    F, k = s.ncol, 2
    i = np.arange(F, dtype=np.float64)
    B = np.ascontiguousarray(np.stack([s.b, s.b * 1.125 + np.cos(i * 0.015)], 1))
    lams = SV.lams_of(s, "m3")
    # (a workgroup owns 256 rows, 2 elements per thread in the flat kernels: the whole panel of scheme 0 runs into a second grid
    #  stride of the kernels that take sums and of the flat ones, a slice of a third of it stays within one)
    assert F > M.RED_BLOCKS * M.RED_THREADS
    dist = DV.Dist(L, s, 3, False)
    try:
        bounds = dist.bounds_t()
        assert [b - a for a, b in zip(bounds, bounds[1:])] == [87381, 87382, 87382] or min(b - a for a, b in zip(bounds, bounds[1:])) > 65536, bounds
        t_csr = DV.sorted_t(dist, s)
        for scheme in (0, 1):
            with G.options(strict_order=1, dist_cg_scheme=scheme):
                got = DV.dmscgn(L, dist, s, B, lams, 3, hbm=scheme == 1, ldx=F * k + 3 * scheme)
            assert np.isfinite(got[0]).all(), scheme
            _assert_model(f"fs_dist_mscgn scheme {scheme} k 2 m3 cap 3 on binary_F262145, bounds {bounds}", got,
                          _model(s, B, lams, 3, t_csr, bounds if scheme == 1 else None))
            assert all(i.iterations == 3 and i.converged == 0 for row in got[1] for i in row), [(i.iterations, i.converged) for row in got[1] for i in row]
    finally:
        dist.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def _repeats(a, b):
    return bool(M.same_bits(a[0], b[0]).all()) and [i.iterations for i in a[1]] == [i.iterations for i in b[1]]


@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_one_lambda_is_fs_dist_pcgn_lambdas_and_fs_dist_pcgn(L, mode):
    for name in ("valued", "binary_F65", "control_seed0"):
        s = DV.ALL[name]
        dist = DV.Dist(L, s, 3, False)
        try:
            for k in (1, 3, 8):
                B = SV.columns(s, k)
                for cap in (0, 5):
                    for scheme in (1, 0):
                        with G.mode_options(mode), G.options(dist_cg_scheme=scheme):
                            if scheme == 1:
                                want, again = [DV.dnl(L, dist, s, B, [s.lam] * k, P.PRECOND_NONE, max_iter=cap) for _ in range(2)]
                            else:
                                want, again = [DV.dpcgn(L, dist, s, B, P.PRECOND_NONE, max_iter=cap) for _ in range(2)]
                            X, infos, cols, _ = DV.dmscgn(L, dist, s, B, [s.lam], cap)
                        what = (name, mode, scheme, k, cap)
                        repeats = _repeats(want, again)
                        assert repeats or (mode == "cg_fixed_order=0" and k > 1), (what, "the right-hand solver does not repeat its bits")
                        if not repeats:                                  # nothing to be equal to
                            continue
                        assert M.same_bits(X[0], want[0]).all(), (what, int((~M.same_bits(X[0], want[0])).sum()))
                        for j in range(k):
                            g, w, (st, shifts) = infos[0][j], want[1][j], cols[j]
                            assert (g.iterations, g.converged) == (w.iterations, w.converged), (what, j, g.iterations, g.converged, w.iterations, w.converged)
                            assert M.same_bits(g.rnorm, w.rnorm)[0] and M.same_bits(g.bnorm, w.bnorm)[0], (what, j)
                            assert shifts["z"][0] == 1.0 and shifts["pslot"][0] == -1.0 and st["iter"] == w.iterations, (what, j)
        finally:
            dist.close()


@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_one_column_is_fs_dist_mscg(L, mode):
    for name, ladder, cap in (("fixture_100x50", "m8", 0), ("binary_F65", "m3", 5), ("valued", "m8", 0), ("zero_rhs", "m3", 0),
                              ("control_seed0", "m8", 0), ("powerlaw_seed0", "m3", 0), ("lambda0_empty_column", "m8", 5)):
        s = DV.MSCG_ALL[name]
        lams = SV.lams_of(s, ladder)
        dist = DV.Dist(L, s, 3, False)
        try:
            for scheme in (0, 1):
                with G.mode_options(mode), G.options(dist_cg_scheme=scheme):
                    x, info, st, shifts = DV.dmscg(L, dist, s, lams, cap)
                    X, infos, cols, _ = DV.dmscgn(L, dist, s, s.b.reshape(-1, 1), lams, cap, hbm=scheme == 1)
                SV.assert_ladder_column(f"fs_dist_mscgn with k = 1 vs fs_dist_mscg [{mode}] scheme {scheme} {ladder} cap {cap} on {name}", X[:, :, 0],
                                   [row[0] for row in infos], cols[0], x, info, SV.written(st), shifts)
        finally:
            dist.close()


@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_pairs_of_the_smallest_lambda_are_fs_dist_cg(L, mode):
    """k = 1 in every mode (the products are the single-vector ones); k = 4 where the k-column product has the single-vector product's
    bits: strict_order"""
    for name in ("fixture_100x50", "valued", "control_seed0"):
        s = DV.ALL[name]
        dist = DV.Dist(L, s, 3, False)
        try:
            for k in ((1, 4) if mode == "strict_order" else (1,)):
                B = SV.columns(s, k)
                for scheme in (0, 1):
                    for ladder in ("m3", "m8"):
                        lams = SV.lams_of(s, ladder)
                        base = [i for i, lam in enumerate(lams) if lam == min(lams)]
                        assert min(lams) == s.lam and len(base) == {"m3": 2, "m8": 1}[ladder]
                        with G.mode_options(mode), G.options(dist_cg_scheme=scheme):
                            X, infos, cols, _ = DV.dmscgn(L, dist, s, B, lams)
                            for j in SV.nonzero_columns(B):
                                xc, itc, stc = dist.cg(False, b=B[:, j])
                                for i in base:
                                    what = (name, mode, scheme, k, ladder, i, j)
                                    assert M.same_bits(X[i][:, j], xc).all() and infos[i][j].iterations == itc, (what, M.mismatch(X[i][:, j], xc, infos[i][j].iterations, itc))
                                    assert infos[i][j].converged == int(stc["done"]) and cols[j][1]["z"][i] == 1.0 and cols[j][1]["pslot"][i] == -1.0, what
        finally:
            dist.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DV.MSCG_RECIPES0))
def test_large_shifts_freeze_on_slices(L, name):
    s = DV.MSCG_RECIPES0[name]
    lams = [s.lam, s.lam + 1e6, s.lam + 1e9]
    B = SV.columns(s, 4)
    dist = DV.Dist(L, s, 3, False)
    try:
        bounds = dist.bounds_t()
        t_csr = DV.sorted_t(dist, s)
        with G.options(strict_order=1, dist_cg_scheme=1):
            got = DV.dmscgn(L, dist, s, B, lams, tol=1e-14, hbm=True)
            X, infos, cols, _ = got
            counts = [[i.iterations for i in row] for row in infos]
            print(f"{name}: counts {counts}")
            assert np.isfinite(X).all() and all(np.isfinite(v).all() for _, shifts in cols for v in shifts.values()), name
            assert all(i.converged == 1 for row in infos for i in row), (name, counts)
            _assert_model(f"fs_dist_mscgn scheme 1 large shifts on {name}", got, _model(s, B, lams, 0, t_csr, bounds, tol=1e-14))
            assert max(counts[2]) + 2 < max(counts[0]) and max(counts[1]) + 2 < max(counts[0]), counts
            for i in (2, 1):                                         # the solve capped where shift i lost its last pair: its panel is final there
                capped = DV.dmscgn(L, dist, s, B, lams, max(counts[i]) + 1, tol=1e-14)
                assert [c.iterations for c in capped[1][i]] == counts[i] and all(c.converged == 1 for c in capped[1][i]), (i, counts[i])
                assert M.same_bits(capped[0][i], X[i]).all(), (name, i, "a shift without a live pair was written again")
    finally:
        dist.close()


def test_a_nan_column_stays_in_its_column(L):
    s = DV.ALL["binary_F65"]
    lams = SV.lams_of(s, "m3")
    B = SV.columns(s, 5)
    clean = B.copy()
    B[7, 3] = np.nan
    dist = DV.Dist(L, s, 3, False)
    try:
        bounds = dist.bounds_t()
        t_csr = DV.sorted_t(dist, s)
        for scheme in (0, 1):
            with G.options(strict_order=1, dist_cg_scheme=scheme):
                want = DV.dmscgn(L, dist, s, clean, lams, 5)
                got = DV.dmscgn(L, dist, s, B, lams, 5, hbm=scheme == 1)            # FS_OK: the ranks agree about the NaN column too
                alone = DV.dmscg(L, dist, s, lams, 5, b=B[:, 3])
            X, infos, cols, st = got
            for j in (0, 1, 2, 4):
                what = (scheme, j)
                assert M.same_bits(X[:, :, j], want[0][:, :, j]).all() and np.isfinite(X[:, :, j]).all(), what
                assert [tuple(row[j].iterations for row in infos)] == [tuple(row[j].iterations for row in want[1])], what
                assert S.shifts_mismatch(cols[j][1], want[2][j][1]) is None, what
            _assert_model(f"fs_dist_mscgn scheme {scheme} with a NaN column", got, _model(s, B, lams, 5, t_csr, bounds if scheme == 1 else None),
                          columns=(0, 1, 2, 4))
            # fs_mscg's freeze rule holds per pair: a NaN fails rn > stop, so the pairs end unconverged, at fs_dist_mscg's count
            assert all(row[3].converged == 0 for row in infos) and [row[3].iterations for row in infos] == [i.iterations for i in alone[1]], scheme
            assert all(cols[3][1]["live"] == 0.0) and all(cols[3][1]["converged"] == 0.0), scheme
    finally:
        dist.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DV.MSCG_RECIPES0))
def test_default_mode_ladder_within_the_bars(L, name):
    s = DV.MSCG_RECIPES0[name]
    lams = SV.lams_of(s, "m8")
    B = SV.columns(s, 4)
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), s.t_csr_coo())
    dist = DV.Dist(L, s, 3, False)
    try:
        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                runs = [DV.dmscgn(L, dist, s, B, lams, hbm=bool(run)) for run in range(2)]
            X, infos, _, _ = runs[0]
            for i, lam in enumerate(lams):
                for j in range(4):
                    info, x, nb = infos[i][j], X[i][:, j], float(np.linalg.norm(B[:, j]))
                    res = float(np.linalg.norm(atm(am(x)) + lam * x - B[:, j]) / nb) if nb else 0.0
                    what = (name, scheme, i, j, lam, info.iterations, res)
                    assert info.converged == 1, what
                    assert res <= 2 * s.tol, what
                    assert info.rnorm <= s.tol * info.bnorm, what
            print(f"{name} scheme {scheme}: counts {[[i.iterations for i in row] for row in infos]}")
            assert all(row[2].iterations == 0 for row in infos) and M.same_bits(X[:, :, 2], np.zeros(X[:, :, 2].shape)).all()
            # fixed-order products: a solve repeats its bits
            assert M.same_bits(runs[1][0], X).all(), (name, scheme)
            assert [[i.iterations for i in row] for row in runs[1][1]] == [[i.iterations for i in row] for row in infos], (name, scheme)
    finally:
        dist.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("three_eigenvalues", "fixture_100x50", "control_seed0"))
def test_sharded_products_per_solve(L, name):
    s = DV.MSCG_ALL[name]
    F = s.ncol
    dist = DV.Dist(L, s, 3, False)
    try:
        for scheme, per_iter in ((0, 2), (1, 1)):
            with G.options(strict_order=1, dist_cg_scheme=scheme):
                for k in (1, 3):
                    B = SV.columns(s, k)
                    for ladder, max_iter in (("m1", 0), ("m8", 0), ("m3", 2)):
                        n, (X, infos, _, st) = DV.counted(L, lambda: DV.dmscgn(L, dist, s, B, SV.lams_of(s, ladder), max_iter))
                        at_start = st["done"] == 1.0 and st["iter"] == 0.0 and bool(M.same_bits(X, np.zeros(X.shape)).all())
                        what = (name, scheme, k, ladder, max_iter, n, st["iter"], st["done"], at_start)
                        print(*what)
                        assert st["iter"] == max(i.iterations for row in infos for i in row), what
                        assert n == per_iter * DV.loops(max_iter or F, int(st["iter"]), at_start), what
                    for tol, Bz in ((s.tol, np.zeros_like(B)), (1.0, B), (2.5, B)):          # done at the start: B = 0, tol >= 1
                        n, (X, infos, _, st) = DV.counted(L, lambda: DV.dmscgn(L, dist, s, Bz, SV.lams_of(s, "m3"), tol=tol, hbm=tol == 1.0))
                        assert n == 0, (name, scheme, k, tol, n)
                        assert all(i.converged == 1 and i.iterations == 0 for row in infos for i in row), (name, scheme, k, tol)
                        assert M.same_bits(X, np.zeros(X.shape)).all() and not np.signbit(X).any() and st["iter"] == 0.0, (name, scheme, k, tol)
    finally:
        dist.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_statuses(L):
    from libfastsparse_amd import capi
    s = DV.MSCG_RECIPES0["control_seed0"]
    with contextlib.closing(DV.Dist(L, s, 3, False)) as dist, DV.handle_without_transpose(L, dist, s) as M_not:
        F, k, m = s.ncol, 3, 3
        B = SV.columns(s, k)
        X = (SV.GAP_BITS + np.arange(16 * (F * k + 3), dtype=np.int64)).view(np.float64)      # quiet NaNs, each tagged with its place
        bits = X.view(np.int64).copy()
        lams = [s.lam * 3, s.lam, s.lam * 10]

        def call(M_=dist.M, X_=X.ctypes.data, ldx=F * k, b_=B.ctypes.data, k_=k, m_=m, lam="default", tol=1e-8, max_iter=0, info=None):
            if lam == "default":
                lam = lams + [1.0] * (max(m_, m) - m)
            arr = None if lam is None else (C.c_double * len(lam))(*lam)
            return L.fs_dist_mscgn(M_, X_, ldx, b_, k_, m_, arr, tol, max_iter, info)

        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                bad = {"NULL M": call(M_=None), "NULL X": call(X_=None), "NULL B": call(b_=None), "NULL lambda": call(lam=None),
                       "k 0": call(k_=0), "k -1": call(k_=-1), "k 33": call(k_=N.MAX_RHS + 1, ldx=F * 33), "m 0": call(m_=0), "m -1": call(m_=-1),
                       "m 17": call(m_=17), "ldx < F k": call(ldx=F * k - 1), "ldx F": call(ldx=F), "ldx 0": call(ldx=0),
                       "tol < 0": call(tol=-1e-8), "tol NaN": call(tol=float("nan")), "tol -inf": call(tol=float("-inf")),
                       "lambda NaN": call(lam=[1.0, float("nan"), 2.0]), "lambda inf": call(lam=[float("inf"), 1.0, 2.0]),
                       "lambda -inf": call(lam=[1.0, 2.0, float("-inf")]),
                       "bad arguments on a handle without a transpose": call(M_=M_not, m_=0),
                       "a bad lambda on a handle without a transpose": call(M_=M_not, lam=[1.0, float("nan"), 2.0])}
                assert all(rc == FS_ERR_ARG for rc in bad.values()), (scheme, bad)
                assert L.fs_last_error()
                assert call(M_=M_not) == FS_ERR_NO_TRANSPOSE
                SV.refused_call_leaves(X, bits)
                assert call(tol=0.0, max_iter=2) == FS_OK            # tol = 0 is legal: the cap ends it (info NULL is legal too)
                assert call(m_=16, ldx=F * k + 3) == FS_OK
                infos = (capi.PcgInfo * (m * k))()
                assert call(tol=0.0, max_iter=2, info=infos) == FS_OK
                assert [i.iterations for i in infos] == [2, 2, 0] * 3 and [i.converged for i in infos] == [0, 0, 1] * 3
                assert call(lam=[-0.25, s.lam, 0.0], max_iter=3) == FS_OK   # a negative lambda is the caller's business
                X.view(np.int64)[:] = bits


def test_a_product_error_is_passed_through(L):
    """fs_matrix_release_csr on ONE rank's shard of A': under strict_order a product reads the plain CSR, so the solve ends with
    FS_ERR_RELEASED and the product's message, X untouched; outside strict_order the kept copy serves and the solve is the one from
    before the release"""
    s = SV.RECIPES["scaled_seed0"]                                    # (plain CG does not converge on it: the solves run under a cap)
    lams = SV.lams_of(s, "m3")
    arr = (C.c_double * len(lams))(*lams)
    k = 2
    B = SV.columns(s, k)
    with G.options(binning=2, bin_flags=64):                           # kept two-pass copies: there is something to release for
        dist = DV.Dist(L, s, 3, False)
    try:
        before = {}
        for scheme in (0, 1):
            with G.options(dist_cg_scheme=scheme):
                before[scheme] = DV.dmscgn(L, dist, s, B, lams, 20)
                assert np.isfinite(before[scheme][0]).all()
        assert L.fs_matrix_release_csr(L.fs_dist_matrix_shard(dist.M, 1, 1)) == 1
        for scheme in (0, 1):
            X = np.full(len(lams) * s.ncol * k, np.nan)
            bits = X.view(np.int64).copy()
            with G.options(strict_order=1, dist_cg_scheme=scheme):
                assert L.fs_dist_mscgn(dist.M, X.ctypes.data, s.ncol * k, B.ctypes.data, k, len(lams), arr, s.tol, 20, None) == FS_ERR_RELEASED, scheme
                assert b"fs_matrix_release_csr" in L.fs_last_error()
            SV.refused_call_leaves(X, bits, (scheme, "a refused solve wrote to X"))
            with G.options(dist_cg_scheme=scheme):
                after = DV.dmscgn(L, dist, s, B, lams, 20)              # the kept copy needs no plain array
            _assert_same_solve(("after the release", scheme), after, before[scheme])
    finally:
        dist.close()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (3, 4))
def test_guard_zones(L, k):
    """X (packed and padded) and B in HBM inside guard zones, 16-byte aligned and 8 bytes off: guards untouched, B unchanged, the gaps
    between the panels keep their bits, and the solution does not depend on where X lies"""
    import torch
    from libfastsparse_amd import capi
    mem = LC.TorchMem()
    s = DV.MSCG_RECIPES0["powerlaw_seed0"]
    F = s.ncol
    ne = F * k
    B = SV.columns(s, k)
    dist = DV.Dist(L, s, 3, False)
    try:
        gx, gb = LC.Guarded(mem, "X of fs_dist_mscgn", 8 * (ne + 3)), LC.Guarded(mem, "B of fs_dist_mscgn", ne)
        for scheme in (0, 1):
            for ladder, cap in (("m1", 0), ("m3", 5), ("m8", 0)):
                lams = SV.lams_of(s, ladder)
                m = len(lams)
                ref = None
                for ldx in (ne, ne + 3):
                    for off in (0, 1):
                        mem.put(gb.place(ne, off ^ (ldx & 1)), B.reshape(-1))
                        n = (m - 1) * ldx + ne
                        mem.fill_bits(gx.place(n, off), SV.GAP_BITS)
                        infos = (capi.PcgInfo * (m * k))()
                        with G.options(dist_cg_scheme=scheme):
                            capi.check(L.fs_dist_mscgn(dist.M, gx.view.data_ptr(), ldx, gb.view.data_ptr(), k, m, (C.c_double * m)(*lams), s.tol, cap,
                                                       infos), "fs_dist_mscgn")
                        torch.cuda.synchronize()
                        what = (k, scheme, ladder, cap, ldx, off)
                        bad = mem.first_bad_guard([gx, gb])
                        assert bad is None, (what, bad.first_broken())
                        assert mem.eq(gb.view, mem.const(B.reshape(-1))), (what, "B changed")
                        X, gaps = SV.split_rows_and_gaps(mem.get(gx.view), m, ne, ldx)
                        assert (gaps.view(np.int64) == SV.GAP_BITS).all(), (what, "a gap between the panels was written")
                        assert np.isfinite(X).all(), what
                        if not cap:
                            assert all(i.converged == 1 for i in infos), (what, [i.iterations for i in infos])
                        if ref is None:
                            ref = X
                        assert M.same_bits(X, ref).all(), (what, "the solution depends on where X lies")
    finally:
        dist.close()


def test_interleaved_solves_share_the_work_space_and_give_it_back(L):
    """fs_dist_mscgn at k = 3, fs_dist_mscg, fs_dist_pcgn_lambdas at k = 5, then fs_dist_mscgn at k = 8 with more shifts (the panels are
    re-made, not overrun), both schemes, interleaved on one handle under strict_order: each has its own model's bits, first and again
    between the others; after fs_dist_matrix_destroy free device memory is back where it was before the handle existed, within one
    solve's work space"""
    import _dist_pcgn_lambdas_model as DNL
    import _pcgn_lambdas_model as NL
    s = DV.MSCG_RECIPES0["control_seed0"]
    B3, B5, B8 = SV.columns(s, 3), SV.columns(s, 5), SV.columns(s, 8)
    m3, m8, l5 = SV.lams_of(s, "m3"), SV.lams_of(s, "m8"), NL.rungs(s, 5)
    ranks = 3

    def kinds(dist):
        t_csr, bounds = DV.sorted_t(dist, s), dist.bounds_t()

        def mn(scheme, B, lams, cap, **kw):
            def run():
                with G.options(strict_order=1, dist_cg_scheme=scheme):
                    got = DV.dmscgn(L, dist, s, B, lams, cap, **kw)
                _assert_model(("interleaved fs_dist_mscgn", scheme, B.shape[1], len(lams), cap), got,
                              _model(s, B, lams, cap, t_csr, bounds if scheme == 1 else None))
                return got[0]
            return run

        def ms(scheme, lams):
            def run():
                with G.options(strict_order=1, dist_cg_scheme=scheme):
                    got = DV.dmscg(L, dist, s, lams)
                DV.assert_dmscg_model(("interleaved fs_dist_mscg", scheme), got, DV.dmscg_model(s, "m3", 0, t_csr, bounds if scheme == 1 else None, lams=lams))
                return got[0]
            return run

        def nl(scheme):
            def run():
                with G.options(strict_order=1, dist_cg_scheme=scheme):
                    got = DV.dnl(L, dist, s, B5, l5, P.PRECOND_JACOBI)
                DV.assert_dnl_model(("interleaved fs_dist_pcgn_lambdas", scheme), got,
                                  DNL.run(s, B5, l5, P.PRECOND_JACOBI, t_csr=t_csr, bounds=bounds if scheme == 1 else None, cache=DV.DNL_CACHE))
                return got[0]
            return run

        return [mn(1, B3, m3, 0), ms(1, m3), nl(1), mn(1, B8, m8, 0, hbm=True), mn(0, B3, m3, 5, ldx=s.ncol * 3 + 3), ms(0, m3), nl(0),
                mn(0, B8, m8, 0), mn(1, B3, m8, 5)]

    def unchecked(dist):
        for scheme in (1, 0):
            with G.options(dist_cg_scheme=scheme):
                DV.dmscgn(L, dist, s, B3, m3)
                DV.dmscgn(L, dist, s, B8, m8)

    # one solve's work space, the larger scheme (replicate), k = 8, the m8 ladder: per rank the m X_i and the nslots P_i of F k doubles,
    # R, B, X of fs_dist_pcgn's, the partials and the scalars
    k, m, nslots = 8, 8, 7
    one_solve = 8 * ranks * ((m + nslots + 3) * k * s.ncol + 2048 * k + 9344)
    DV.interleaved_then_memory_back(L, s, ranks, kinds, 7, one_solve, unchecked=unchecked)


# ---- 10 --------------------------------------------------------------------------------------------------------------------
_CutPair = DV.CutPair


@pytest.mark.parametrize("name", list(DN.DIFFERING_BOUNDS))
def test_pair_handle(L, name):
    """A' in the caller's entry order, cut where _dist_mscg_model.DIFFERING_BOUNDS cuts it: both schemes are the models on that A' and
    those bounds, which tell the schemes apart"""
    import _dist_pair as DPair
    s, B8, _ = N.recipe8(name.split("_")[0])
    assert s.name == name
    want_bounds = DN.DIFFERING_BOUNDS[name]
    pd = _CutPair(L, s, want_bounds)
    try:
        bounds = pd.bounds_t()
        assert bounds == want_bounds, (bounds, want_bounds)
        t = pd.t_csr()
        assert DPair.same_arrays(t, s.t_csr_coo()), (name, "the shards of A' are not the caller's arrays")
        for k, ladder, cap in ((8, "m3", 0), (3, "m8", 5)):
            B = np.ascontiguousarray(B8[:, :k])
            lams = SV.lams_of(s, ladder)
            whole, sliced = _model(s, B, lams, cap, t), _model(s, B, lams, cap, t, bounds)
            nz = SV.nonzero_columns(B)
            differ = DN.differing_columns(sliced, whole)
            print(f"{name} k {k} {ladder} cap {cap}: columns whose bits differ between the schemes' models {differ} of the non-zero {nz}")
            assert 2 * len(differ) >= len(nz), (name, k, ladder, cap, differ)
            for scheme in (0, 1):
                with G.options(strict_order=1, dist_cg_scheme=scheme):
                    got = DV.dmscgn(L, pd, s, B, lams, cap, hbm=scheme == 1, ldx=s.ncol * k + 3 * scheme)
                _assert_model(f"fs_dist_mscgn scheme {scheme} k {k} {ladder} cap {cap} on a pair, bounds {bounds}, on {name}", got,
                              sliced if scheme == 1 else whole)
    finally:
        pd.close()
