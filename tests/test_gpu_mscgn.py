"""fs_mscgn against the CPU model of its columns (tests/_mscgn_model.py: column j is the model of fs_mscg on B[:, j]), against fs_mscg
and against fs_pcgn on the device, on the harness of tests/_solvers.py.

1  strict_order: X, every fs_pcg_info and every column's st[] / ms[] have the model's bits -- k in {1, 2, 3, 4, 5, 7, 8, 16, 17, 32}, one
   lambda, three with the minimum twice, the ladder of eight (shuffled) and sixteen, caps 0 and 5; a duplicate column has identical
   bits, a zero column is +0.0 in 0 iterations; also on more than one grid stride per column.
2  strict_order: column j of every panel is fs_mscg on the same handles with B[:, j], bit for bit, counts included.
3  every mode: k = 1 IS fs_mscg on the same handles, bit for bit: X, infos and the state.
4  every mode: m = 1 IS fs_pcgn with FS_PRECOND_NONE from a cold start on the same handles, bit for bit (k in {1, 3, 8}, caps 0 and 5),
   wherever fs_pcgn repeats its own bits.
5  default modes on the control / powerlaw recipes with the ladder of eight and k = 4: every pair converged, true residual (the
   oracle's products) <= 2 tol ||b_j||, rnorm <= tol bnorm (test_gpu_mscg.py test 4's bars); a fixed-order solve repeats its bits.
6  strict_order: a NaN in one column of B changes no bit of another column's pairs; that column's pairs end unconverged.
7  statuses: every FS_ERR_ARG and FS_ERR_RELEASED leaves all of X untouched; info = NULL and tol = 0 with a cap are legal.
8  guard zones around X and B, ldx = F k and F k + 3, 16-byte aligned and 8 bytes off, k = 3 and 4: guards and gaps keep their bits, B
   is unchanged, the result 8 bytes off has the aligned one's bits.
9  the solve does the one-time work of the k-column products itself and leaks no work space.
Tests 1, 2, 6 and 8 run on both values of option "pcgn_kernel" (the kernels that take the per-column sums read it)."""
import copy
import ctypes as C

import numpy as np
import pytest

import _cg_model as M
import _gpu as G
import _lifecycle as LC
import _mscg_model as S
import _mscgn_model as SN
import _pcg_model as P
import _solvers as SV
from _gpu import FS_ERR_ARG, FS_ERR_RELEASED, FS_OK, L  # noqa: F401

pytestmark = pytest.mark.gpu

SYSTEMS10 = ("fixture_100x50", "binary_F1", "binary_F63", "binary_F64", "binary_F65", "binary_F257", "valued", "three_eigenvalues",
             "zero_rhs", "lambda0_empty_column")
# (system, k, ladder, cap): every k and every ladder meets two systems or more, every system two values of k or more
STRICT_SET = [("fixture_100x50", 1, "m8", 0), ("fixture_100x50", 8, "m3", 5), ("fixture_100x50", 32, "m16", 0),
              ("binary_F1", 2, "m1", 0), ("binary_F1", 17, "m3", 0), ("binary_F1", 32, "m8", 5),
              ("binary_F63", 3, "m16", 0), ("binary_F63", 16, "m1", 5),
              ("binary_F64", 4, "m8", 0), ("binary_F64", 7, "m3", 5), ("binary_F64", 32, "m1", 0),
              ("binary_F65", 5, "m16", 5), ("binary_F65", 17, "m8", 0), ("binary_F65", 16, "m3", 0),
              ("binary_F257", 7, "m8", 0), ("binary_F257", 2, "m16", 0),
              ("valued", 8, "m8", 0), ("valued", 3, "m3", 5),
              ("three_eigenvalues", 16, "m16", 0), ("three_eigenvalues", 1, "m3", 0), ("three_eigenvalues", 5, "m1", 0),
              ("zero_rhs", 4, "m3", 0), ("zero_rhs", 8, "m8", 5),
              ("lambda0_empty_column", 2, "m8", 0), ("lambda0_empty_column", 5, "m3", 5), ("lambda0_empty_column", 4, "m16", 0)]
LARGE_CASE = ("binary_F262145", 2, "m3", 0)                            # more than one grid stride per column
_MODEL_CACHE = {}
_COUNTS_SEEN = []                                                      # per strict case: the counts of the smallest lambda, by column


def test_the_strict_set_covers_what_it_should():
    for k in SV.KS:
        assert len({n for n, kk, _, _ in STRICT_SET if kk == k}) >= 2, k
    for ladder in SV.LADDERS:
        assert len({n for n, _, l, _ in STRICT_SET if l == ladder}) >= 2, ladder
    for name in SYSTEMS10:
        assert len({k for n, k, _, _ in STRICT_SET if n == name}) >= 2, name
    assert {n for n, _, _, _ in STRICT_SET} == set(SYSTEMS10) and {k for _, k, _, _ in STRICT_SET} == set(SV.KS)
    assert {c for _, _, _, c in STRICT_SET} == {0, 5} and set(SV.LADDERS) == {"m1", "m3", "m8", "m16"}
    assert {len(SV.LADDERS[l]) for l in SV.LADDERS} == {1, 3, 8, 16} and SV.LADDERS["m3"].count(min(SV.LADDERS["m3"])) == 2
    s = SV.MSCG_ALL[LARGE_CASE[0]]
    assert s.ncol > M.RED_BLOCKS * M.RED_THREADS and LARGE_CASE[1:3] == (2, "m3")


def _with_b(s, b):
    t = copy.copy(s)
    t.b = np.ascontiguousarray(b)
    return t


def _column_infos(infos, j):
    return [row[j] for row in infos]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def _strict_case(L, name, k, ladder, cap, kernel):
    s = SV.MSCG_ALL[name]
    lams = SV.lams_of(s, ladder)
    B = SV.columns(s, k)
    model = SN.run(s, B, lams, max_iter=cap, cache=_MODEL_CACHE)
    with G.options(strict_order=1, pcgn_kernel=kernel):
        A, At = SV.handles(L, s)
        X, infos, cols = SV.mscgn_run(L, A, At, s, B, lams, cap)
    assert X.shape == (len(lams), s.ncol, k) and len(infos) == len(lams) and all(len(r) == k for r in infos)
    for j in range(k):
        c = model.columns[j]
        SV.assert_ladder_column(f"fs_mscgn {ladder} cap {cap} k {k} on {name}, column {j}", X[:, :, j], _column_infos(infos, j), cols[j], c.X, c.infos,
                       c.state, c.shifts)
        if cap:
            assert all(i.iterations <= cap for i in _column_infos(infos, j))
    if k >= 2:
        assert M.same_bits(X[:, :, 1], X[:, :, 0]).all(), (name, k, ladder, "the duplicate column")
        assert [i.iterations for i in _column_infos(infos, 1)] == [i.iterations for i in _column_infos(infos, 0)]
    if k >= 3:
        assert all(i.iterations == 0 and i.converged == 1 for i in _column_infos(infos, 2)), (name, k, ladder, "the zero column")
        assert M.same_bits(X[:, :, 2], np.zeros((len(lams), s.ncol))).all() and not np.signbit(X[:, :, 2]).any()
    base = int(np.argmin(lams))
    _COUNTS_SEEN.append([infos[base][j].iterations for j in range(k)])


@pytest.mark.parametrize("kernel", SV.KERNELS, ids=[f"pcgn_kernel{v}" for v in SV.KERNELS])
@pytest.mark.parametrize("name,k,ladder,cap", STRICT_SET, ids=[f"{n}-k{k}-{l}-cap{c}" for n, k, l, c in STRICT_SET])
def test_fs_mscgn_strict_is_the_model(L, name, k, ladder, cap, kernel):
    _strict_case(L, name, k, ladder, cap, kernel)


def test_fs_mscgn_strict_is_the_model_on_more_than_one_grid_stride(L):
    for kernel in SV.KERNELS:
        _strict_case(L, *LARGE_CASE, kernel)


def test_columns_finish_at_different_iterations(L):
    """some strict case has live columns (not the zero one) that end at different counts: the live mask and the freezing are at work"""
    if not _COUNTS_SEEN:
        _strict_case(L, "valued", 8, "m8", 0, 0)
    assert any(len({c for c in counts if c > 0}) >= 2 for counts in _COUNTS_SEEN), _COUNTS_SEEN


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", SV.KERNELS, ids=[f"pcgn_kernel{v}" for v in SV.KERNELS])
@pytest.mark.parametrize("name,k,ladder,cap", [("fixture_100x50", 5, "m8", 0), ("valued", 3, "m16", 0), ("binary_F257", 4, "m3", 5),
                                               ("powerlaw_seed0", 7, "m8", 0)])
def test_columns_are_fs_mscg_on_the_same_handles(L, name, k, ladder, cap, kernel):
    s = SV.MSCG_ALL[name]
    lams = SV.lams_of(s, ladder)
    B = SV.columns(s, k)
    with G.options(strict_order=1, pcgn_kernel=kernel):
        A, At = SV.handles(L, s)
        alone = [SV.mscg_run(L, A, At, _with_b(s, B[:, j]), lams, cap) for j in range(k)]
        X, infos, cols = SV.mscgn_run(L, A, At, s, B, lams, cap)
    for j, (x, info, st, shifts) in enumerate(alone):
        SV.assert_ladder_column(f"column {j} of fs_mscgn {ladder} cap {cap} vs fs_mscg on {name}", X[:, :, j], _column_infos(infos, j), cols[j], x, info,
                       SV.written(st), shifts)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_one_column_is_fs_mscg(L, mode):
    for name, ladder, cap in (("fixture_100x50", "m8", 0), ("binary_F65", "m3", 5), ("valued", "m16", 0), ("zero_rhs", "m3", 0),
                              ("control_seed0", "m8", 0), ("powerlaw_seed0", "m8", 0), ("lambda0_empty_column", "m8", 5)):
        s = SV.MSCG_ALL[name]
        lams = SV.lams_of(s, ladder)
        with G.mode_options(mode):
            A, At = SV.handles(L, s)
            x, info, st, shifts = SV.mscg_run(L, A, At, s, lams, cap)
            X, infos, cols = SV.mscgn_run(L, A, At, s, s.b.reshape(-1, 1), lams, cap)
        SV.assert_ladder_column(f"fs_mscgn with k = 1 vs fs_mscg [{mode}] {ladder} cap {cap} on {name}", X[:, :, 0], _column_infos(infos, 0), cols[0], x,
                       info, SV.written(st), shifts)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", (0, 5))
@pytest.mark.parametrize("k", (1, 3, 8))
@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_one_lambda_is_fs_pcgn_without_preconditioner(L, mode, k, cap):
    for name in ("fixture_100x50", "binary_F257", "scaled_seed0", "powerlaw_seed0"):
        s = SV.MSCG_ALL[name]
        B = SV.columns(s, k)
        with G.mode_options(mode):
            A, At = SV.handles(L, s)
            Xp, ip, _, cs = SV.pcgn_run(L, A, At, s, B, P.PRECOND_NONE, max_iter=cap)
            Xq, iq, _, _ = SV.pcgn_run(L, A, At, s, B, P.PRECOND_NONE, max_iter=cap)
            X, infos, cols = SV.mscgn_run(L, A, At, s, B, [s.lam], cap)
        repeats = M.same_bits(Xp, Xq).all() and [i.iterations for i in ip] == [i.iterations for i in iq]
        assert repeats or (mode == "cg_fixed_order=0" and k > 1), (mode, name, k, "fs_pcgn does not repeat its bits")
        if not repeats:                                                # nothing to be equal to
            continue
        what = (mode, name, k, cap)
        assert M.same_bits(X[0], Xp).all(), (what, int((~M.same_bits(X[0], Xp)).sum()))
        for j in range(k):
            g, w, (st, shifts) = infos[0][j], ip[j], cols[j]
            assert g.iterations == w.iterations and g.converged == w.converged, (what, j, g.iterations, g.converged, w.iterations, w.converged)
            assert M.same_bits(g.rnorm, w.rnorm)[0] and M.same_bits(g.bnorm, w.bnorm)[0], (what, j, g.rnorm, g.bnorm, w.rnorm, w.bnorm)
            assert shifts["z"][0] == 1.0 and shifts["pslot"][0] == -1.0 and st["iter"] == w.iterations, (what, j)
            for key in ("rr", "bb", "stop", "rsq", "alpha", "beta"):     # (a slot its column never wrote is 0 in both)
                assert M.same_bits(st[key], cs[j]["rz" if key == "rsq" else key])[0], (what, j, key, st[key], cs[j])


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SV.MSCG_RECIPES))
def test_default_modes_ladder_within_the_bars(L, name):
    s = SV.MSCG_RECIPES[name]
    lams = SV.lams_of(s, "m8")
    B = SV.columns(s, 4)
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), s.t_csr_coo())
    for mode in ("default", "cg_fixed_order=0"):
        with G.mode_options(mode):
            A, At = SV.handles(L, s)
            runs = [SV.mscgn_run(L, A, At, s, B, lams) for _ in range(2)]
        X, infos, _ = runs[0]
        for i, lam in enumerate(lams):
            for j in range(4):
                info, x, nb = infos[i][j], X[i][:, j], float(np.linalg.norm(B[:, j]))
                res = float(np.linalg.norm(atm(am(x)) + lam * x - B[:, j]) / nb) if nb else 0.0
                what = (name, mode, i, j, lam, info.iterations, res)
                assert info.converged == 1, what
                assert res <= 2 * s.tol, what
                assert info.rnorm <= s.tol * info.bnorm, what
        print(f"{name} [{mode}]: counts {[[i.iterations for i in row] for row in infos]}")
        assert all(i.iterations == 0 for i in _column_infos(infos, 2)) and M.same_bits(X[:, :, 2], np.zeros(X[:, :, 2].shape)).all()
        if mode == "default":                                           # fixed-order products: a solve repeats its bits
            assert M.same_bits(runs[1][0], X).all(), name
            assert [[i.iterations for i in row] for row in runs[1][1]] == [[i.iterations for i in row] for row in infos], name


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_a_nan_column_stays_in_its_column(L):
    s = SV.MSCG_ALL["binary_F257"]
    lams = SV.lams_of(s, "m3")
    B = SV.columns(s, 5)
    B[7, 3] = np.nan
    with G.options(strict_order=1):
        A, At = SV.handles(L, s)
        alone = {j: SV.mscg_run(L, A, At, _with_b(s, B[:, j]), lams, 5) for j in range(5)}
        for kernel in SV.KERNELS:
            with G.options(pcgn_kernel=kernel):
                X, infos, cols = SV.mscgn_run(L, A, At, s, B, lams, 5)
            for j, (x, info, st, shifts) in alone.items():
                what = (s.name, kernel, j)
                assert M.same_bits(X[:, :, j], x).all(), what
                SV.assert_infos(what, _column_infos(infos, j), info)
                assert S.shifts_mismatch(cols[j][1], shifts) is None, what
                if j != 3:
                    assert np.isfinite(X[:, :, j]).all(), what
            # fs_mscg's freeze rule holds per pair: a NaN fails rn > stop, so the pairs end unconverged, within the cap
            assert all(i.converged == 0 and i.iterations <= 5 for i in _column_infos(infos, 3)), [(i.iterations, i.converged) for i in _column_infos(infos, 3)]
            assert all(cols[3][1]["live"] == 0.0) and all(cols[3][1]["converged"] == 0.0)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_statuses(L):
    from libfastsparse_amd import capi
    s = SV.MSCG_RECIPES["control_seed0"]
    A, At = SV.handles(L, s)
    st = capi.current_stream()
    F, k, m = s.ncol, 3, 3
    B = G.to_device(SV.columns(s, k))
    bits = LC.PREFILLS["nan"] + np.arange(16 * (F * k + 3), dtype=np.int64)       # quiet NaNs, each tagged with its place
    X = G.to_device(bits.view(np.float64))
    lams = [s.lam * 3, s.lam, s.lam * 10]

    def call(A_=A.h, At_=At.h, X_=X.data_ptr(), ldx=F * k, b_=B.data_ptr(), k_=k, m_=m, lam="default", tol=1e-8, max_iter=0, info=None):
        if lam == "default":
            lam = lams + [1.0] * (max(m_, m) - m)
        arr = None if lam is None else (C.c_double * len(lam))(*lam)
        return L.fs_mscgn(A_, At_, X_, ldx, b_, k_, m_, arr, tol, max_iter, info, st)

    bad = {"NULL A": call(A_=None), "NULL At": call(At_=None), "NULL X": call(X_=None), "NULL B": call(b_=None), "NULL lambda": call(lam=None),
           "At of A's shape": call(At_=A.h), "k 0": call(k_=0), "k -1": call(k_=-1), "k 33": call(k_=33), "m 0": call(m_=0), "m -1": call(m_=-1),
           "m 17": call(m_=17), "ldx < F k": call(ldx=F * k - 1), "ldx F": call(ldx=F), "ldx 0": call(ldx=0), "tol < 0": call(tol=-1e-8),
           "tol NaN": call(tol=float("nan")), "tol -inf": call(tol=float("-inf")), "lambda NaN": call(lam=[1.0, float("nan"), 2.0]),
           "lambda inf": call(lam=[float("inf"), 1.0, 2.0]), "lambda -inf": call(lam=[1.0, 2.0, float("-inf")])}
    assert all(rc == FS_ERR_ARG for rc in bad.values()), bad
    assert L.fs_last_error()
    SV.refused_call_leaves(X, bits)
    assert call(tol=0.0, max_iter=2) == FS_OK                          # tol = 0 is legal: the cap ends it (info NULL is legal too)
    assert call(m_=16, ldx=F * k + 3) == FS_OK
    infos = (capi.PcgInfo * (m * k))()
    assert call(tol=0.0, max_iter=2, info=infos) == FS_OK
    assert [i.iterations for i in infos] == [2, 2, 0] * 3 and [i.converged for i in infos] == [0, 0, 1] * 3
    assert call(lam=[-0.25, s.lam, 0.0], max_iter=3) == FS_OK           # a negative lambda is the caller's business


def test_released_handles(L):
    """FS_ERR_RELEASED before anything is written to X: under strict_order after fs_matrix_release_csr on a kept two-pass A'; for a k
    that was never prepared before the release.  After fs_matrix_restore_csr the same bits return."""
    from libfastsparse_amd import capi
    s = SV.MSCG_RECIPES["powerlaw_seed0"]
    st = capi.current_stream()
    trp, tcc, tvv = s.t_csr_coo()
    lams = SV.lams_of(s, "m3")
    arr = (C.c_double * len(lams))(*lams)
    k = 3
    B = SV.columns(s, k)
    A, _ = SV.handles(L, s)
    with G.options(binning=2, bin_flags=64):                           # a kept two-pass copy: there is something to release for
        At = capi.Matrix.from_csr(s.ncol, s.nrow, G.to_device(trp), G.to_device(tcc), None if tvv is None else G.to_device(tvv))
    assert At.kernel_name() == "two-pass"
    X_before, infos_before, _ = SV.mscgn_run(L, A, At, s, B, lams)        # prepares k = 3
    assert all(i.converged == 1 for row in infos_before for i in row)
    assert At.release_csr() == 1
    X = G.nan_vector(len(lams) * s.ncol * 4)
    bits = X.cpu().numpy().view(np.int64).copy()
    Bd, B4 = G.to_device(B), G.to_device(SV.columns(s, 4))
    with G.options(strict_order=1):
        assert L.fs_mscgn(A.h, At.h, X.data_ptr(), s.ncol * k, Bd.data_ptr(), k, len(lams), arr, s.tol, 0, None, st) == FS_ERR_RELEASED
        assert b"fs_matrix_release_csr" in L.fs_last_error()
    SV.refused_call_leaves(X, bits, "the refused strict solve wrote to X")
    # k = 4 was never prepared on this A': fs_matrix_prepare needs the plain arrays
    assert L.fs_mscgn(A.h, At.h, X.data_ptr(), s.ncol * 4, B4.data_ptr(), 4, len(lams), arr, s.tol, 3, None, st) == FS_ERR_RELEASED
    SV.refused_call_leaves(X, bits, "the refused k = 4 solve wrote to X")
    X_after, infos_after, _ = SV.mscgn_run(L, A, At, s, B, lams)          # the kept copy needs no plain array
    assert M.same_bits(X_after, X_before).all()
    assert [[i.iterations for i in row] for row in infos_after] == [[i.iterations for i in row] for row in infos_before]
    At.restore_csr(G.to_device(trp), G.to_device(tcc), None if tvv is None else G.to_device(tvv))
    with G.options(strict_order=1):
        X_strict, infos_strict, _ = SV.mscgn_run(L, A, At, s, B, lams)
    assert all(i.converged == 1 for row in infos_strict for i in row) and np.isfinite(X_strict).all()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_guard_zones(L):
    """X and B inside guard zones (tests/_lifecycle.py), 16-byte aligned and 8 bytes off, panels packed and padded, both forms of the
    kernels that take sums: guards and gaps untouched, B unchanged, and the result has the bits of the first placement"""
    import torch
    from libfastsparse_amd import capi
    mem = LC.TorchMem()
    st = capi.current_stream()
    gap_bits = LC.PREFILLS["nan"]
    for name in ("control_seed0", "binary_F257"):
        s = SV.MSCG_ALL[name]
        F = s.ncol
        A, At = SV.handles(L, s)
        gx, gb = LC.Guarded(mem, "X of fs_mscgn", 16 * (F * 4 + 3)), LC.Guarded(mem, "B of fs_mscgn", F * 4)
        for kernel, k, ladder, cap in [(v, k, l, c) for v in SV.KERNELS for k in (3, 4) for l, c in (("m1", 0), ("m3", 0), ("m8", 5), ("m16", 0))]:
            lams = SV.lams_of(s, ladder)
            m = len(lams)
            B = SV.columns(s, k)
            ne = F * k
            ref = None
            for ldx in (ne, ne + 3):
                for off in (0, 1):
                    mem.put(gb.place(ne, off ^ (ldx & 1)), B.reshape(-1))
                    n = (m - 1) * ldx + ne
                    mem.fill_bits(gx.place(n, off), gap_bits)
                    infos = (capi.PcgInfo * (m * k))()
                    with G.options(pcgn_kernel=kernel):
                        capi.check(L.fs_mscgn(A.h, At.h, gx.view.data_ptr(), ldx, gb.view.data_ptr(), k, m, (C.c_double * m)(*lams), s.tol, cap,
                                              infos, st), "fs_mscgn")
                    torch.cuda.synchronize()
                    what = (name, kernel, k, ladder, cap, ldx, off)
                    bad = mem.first_bad_guard([gx, gb])
                    assert bad is None, (what, bad.first_broken())
                    assert mem.eq(gb.view, mem.const(B.reshape(-1))), (what, "B changed")
                    X, gaps = SV.split_rows_and_gaps(mem.get(gx.view), m, ne, ldx)
                    assert (gaps.view(np.int64) == gap_bits).all(), (what, "a gap between panels was written")
                    assert np.isfinite(X).all(), what
                    if not cap:
                        assert all(i.converged == 1 for i in infos), (what, [i.iterations for i in infos])
                    # the placement picks 16-byte or 8-byte accesses, never a bit (fixed-order products: a solve repeats its bits)
                    if ref is None:
                        ref = (X, [i.iterations for i in infos])
                    assert M.same_bits(X, ref[0]).all() and [i.iterations for i in infos] == ref[1], (what, "the solution depends on where X lies")


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
def test_the_solve_prepares_the_products_and_leaks_no_work_space(L):
    import torch
    from libfastsparse_amd import capi
    s = SV.MSCG_RECIPES["powerlaw_seed0"]
    arp, acc, avv = s.a_csr()
    trp, tcc, tvv = s.t_csr_coo()
    lams = SV.lams_of(s, "m8")
    # a matrix this small keeps and extends the two-pass copy only under binning = 2; the solver's own options are the defaults
    with G.options(binning=2, bin_flags=64):
        A = capi.Matrix.from_csr(s.nrow, s.ncol, G.to_device(arp), G.to_device(acc), None if avv is None else G.to_device(avv))
        At = capi.Matrix.from_csr(s.ncol, s.nrow, G.to_device(trp), G.to_device(tcc), None if tvv is None else G.to_device(tvv))
        assert A.kernel_name() == "two-pass" and At.kernel_name() == "two-pass"
        assert A.spmm_plan(4) != "k-column two-pass" and At.spmm_plan(4) != "k-column two-pass"
        B = G.to_device(SV.columns(s, 4))
        X = G.nan_vector(len(lams) * s.ncol * 4).view(len(lams), s.ncol, 4)
        free = []
        for _ in range(3):
            infos = capi.mscgn(A, At, X, B, lams, s.tol, 0, capi.current_stream())
            torch.cuda.synchronize()
            free.append(torch.cuda.mem_get_info()[0])
            assert all(i.converged == 1 for row in infos for i in row)
        assert A.spmm_plan(4) == "k-column two-pass" and At.spmm_plan(4) == "k-column two-pass"
        assert free[1] == free[0] and free[2] == free[0], free         # the work space of a solve goes back when it returns
