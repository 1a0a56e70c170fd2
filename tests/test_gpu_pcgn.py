"""fs_pcgn against the CPU model of its columns (tests/_pcgn_model.py: column j is the model of fs_pcg on B[:, j]) and against fs_pcg
on the device, on the harness of tests/_solvers.py.

1  strict_order: X, every fs_pcg_info and the per-column state have the model's bits -- k in {1, 2, 3, 4, 5, 7, 8, 16, 17, 32}, the cases
   of _solvers.CASES (none, Jacobi, a caller's diagonal, warm starts, caps); a duplicate column has identical bits, a zero column is
   x = +0.0 in 0 iterations.
2  strict_order: column j is fs_pcg on the same handles with B[:, j], bit for bit -- on more than one grid stride per column, and from
   a warm start whose columns freeze at different iterations, one of them before the first product.
3  every mode: k = 1 IS fs_pcg on the same handles, bit for bit: x, info and the state.
4  default modes on the eight-column recipes: every column converged, true residual (the oracle's products) <= 2 tol, the count within
   one of the model's, rnorm <= tol bnorm; fixed-order solves repeat their bits (fs_pcg's own bars).
5  strict_order: a NaN in one column of B changes no bit of another column.
6  statuses: every FS_ERR_ARG and FS_ERR_RELEASED leaves X untouched; info = NULL and tol = 0 with a cap are legal.
7  guard zones around X, B and diag, 16-byte aligned and 8 bytes off, k = 3 and 4; the result 8 bytes off has the aligned one's bits.
8  the solve does the one-time work of the k-column products itself.
Tests 1, 2, 5 and 7 run on both forms of the per-iteration kernels (option "pcgn_kernel" 1: a lane per row, 2: staged through LDS)."""
import ctypes as C

import numpy as np
import pytest

import _cg_model as M
import _gpu as G
import _lifecycle as LC
import _pcg_model as P
import _pcgn_model as N
import _solvers as SV
from _gpu import FS_ERR_ARG, FS_ERR_RELEASED, FS_OK, L  # noqa: F401

pytestmark = pytest.mark.gpu

# (system, k, case of CASES): every k meets no preconditioner, Jacobi and a caller's diagonal; every system meets two values of k or more.
# The wide panels go to the systems whose model is quick (the model solves every distinct column in Python)
STRICT_SET = [("fixture_100x50", 1, 0), ("fixture_100x50", 8, 1), ("fixture_100x50", 32, 2),
              ("binary_F1", 2, 0), ("binary_F1", 17, 1), ("binary_F1", 32, 0),
              ("binary_F63", 3, 2), ("binary_F63", 16, 1),
              ("binary_F64", 4, 0), ("binary_F64", 32, 1), ("binary_F64", 7, 4),
              ("binary_F65", 5, 1), ("binary_F65", 17, 2), ("binary_F65", 16, 0),
              ("binary_F257", 7, 2), ("binary_F257", 2, 3),
              ("valued", 8, 0), ("valued", 3, 1),
              ("lambda0_empty_column", 2, 2), ("lambda0_empty_column", 5, 0),
              ("three_eigenvalues", 16, 2), ("three_eigenvalues", 17, 0), ("three_eigenvalues", 7, 1),
              ("zero_rhs", 4, 1), ("zero_rhs", 8, 2), ("zero_rhs", 1, 1),
              ("scaled_seed0", 4, 2), ("scaled_seed0", 5, 6), ("scaled_seed0", 7, 5),
              ("powerlaw_seed0", 1, 6), ("powerlaw_seed0", 3, 4)]
SYSTEMS12 = ("fixture_100x50", "binary_F1", "binary_F63", "binary_F64", "binary_F65", "binary_F257", "valued", "lambda0_empty_column",
             "three_eigenvalues", "zero_rhs", "scaled_seed0", "powerlaw_seed0")
_MODEL_CACHE = {}


def test_the_strict_set_covers_what_it_should():
    met = {(k, SV.CASES[c][1]) for _, k, c in STRICT_SET}
    assert met == {(k, p) for k in SV.KS for p in (P.PRECOND_NONE, P.PRECOND_JACOBI, P.PRECOND_DIAG)}
    for name in SYSTEMS12:
        assert len({k for n, k, _ in STRICT_SET if n == name}) >= 2, name
    assert {n for n, _, _ in STRICT_SET} == set(SYSTEMS12)
    assert {c for _, _, c in STRICT_SET} == set(range(len(SV.CASES)))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", SV.KERNELS, ids=[f"pcgn_kernel{v}" for v in SV.KERNELS])
@pytest.mark.parametrize("name,k,case", STRICT_SET, ids=[f"{n}-k{k}-{SV.CASES[c][0]}" for n, k, c in STRICT_SET])
def test_fs_pcgn_strict_is_the_model(L, name, k, case, kernel):
    s = SV.ALL[name]
    what, precond, warm, max_iter = SV.CASES[case]
    diag = SV.caller_diag(s) if precond == P.PRECOND_DIAG else None
    B = SV.columns(s, k)
    X0 = SV.x0_columns(s, B) if warm else None
    model = N.run(s, B, precond, max_iter=max_iter, X0=X0, diag=diag, cache=_MODEL_CACHE)
    with G.options(strict_order=1, pcgn_kernel=kernel):
        A, At = SV.handles(L, s)
        X, infos, st, cs = SV.pcgn_run(L, A, At, s, B, precond, X0, max_iter, diag)
    assert len(infos) == k
    for j in range(k):
        SV.assert_column((name, k, what, j), X[:, j], infos[j], cs[j], model.X[:, j], model.infos[j], model.columns[j].state)
        if max_iter:
            assert infos[j].iterations <= max_iter
    if k >= 2:
        assert M.same_bits(X[:, 1], X[:, 0]).all() and infos[1].iterations == infos[0].iterations, (name, k, what, "the duplicate column")
    if k >= 3:
        assert infos[2].iterations == 0 and infos[2].converged == 1, (name, k, what, infos[2].iterations)
        assert M.same_bits(X[:, 2], np.zeros(s.ncol)).all(), (name, k, what, "the zero column")
    assert st["iter"] == max(i.iterations for i in infos) and st["done"] == float(all(c["live"] == 0.0 for c in cs)), (name, k, what, st)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def _pcg_column(L, A, At, s, b, precond, x0=None, max_iter=0, tol=None):
    """fs_pcg on one column: x, its info, and the scalars of st[] that such a solve is sure to have written (a solve that is done at
    the start writes neither r.z nor alpha, one without a second iteration no beta: those slots hold what the allocation held)"""
    x, info, st = SV.pcg_run(L, A, At, s, precond, x0, max_iter, tol=tol, b=b)
    if info.iterations == 0:
        st = {k: v for k, v in st.items() if k not in ("rsq", "alpha", "beta")}
    return x, N.Info(info.iterations, info.converged, info.rnorm, info.bnorm), st


def test_columns_are_fs_pcg_on_more_than_one_grid_stride(L):
    s = SV.ALL["binary_F262145"]
    assert s.ncol > M.RED_BLOCKS * M.RED_THREADS
    i = np.arange(s.ncol, dtype=np.float64)
    B = np.stack([s.b, np.cos(i * 0.013) + 0.5 * s.b, np.sin(i * 0.7) * 3.0], 1)
    with G.options(strict_order=1):
        A, At = SV.handles(L, s)
        alone = [_pcg_column(L, A, At, s, B[:, j], P.PRECOND_JACOBI) for j in range(3)]
        for kernel in SV.KERNELS:
            with G.options(pcgn_kernel=kernel):
                X, infos, _, cs = SV.pcgn_run(L, A, At, s, B, P.PRECOND_JACOBI)
            for j, (x, info, st) in enumerate(alone):
                assert info.converged == 1 and info.iterations > 0
                SV.assert_column((s.name, kernel, j), X[:, j], infos[j], cs[j], x, info, st)


def test_warm_columns_freeze_at_different_iterations(L):
    """X0 columns from fs_pcg: not run at all, capped at 3, run to a hundredth of tol -- the last is done before the first product"""
    s = SV.ALL["valued"]
    i = np.arange(s.ncol, dtype=np.float64)
    B = np.stack([s.b, s.b * 0.5 + np.cos(i * 0.05), np.sin(i * 0.3) + 0.25 * s.b], 1)
    with G.options(strict_order=1):
        A, At = SV.handles(L, s)
        X0 = np.zeros(B.shape)
        X0[:, 1] = _pcg_column(L, A, At, s, B[:, 1], P.PRECOND_JACOBI, max_iter=3)[0]
        X0[:, 2] = _pcg_column(L, A, At, s, B[:, 2], P.PRECOND_JACOBI, tol=s.tol * 1e-2)[0]
        alone = [_pcg_column(L, A, At, s, B[:, j], P.PRECOND_JACOBI, x0=X0[:, j]) for j in range(3)]
        for kernel in SV.KERNELS:
            with G.options(pcgn_kernel=kernel):
                X, infos, _, cs = SV.pcgn_run(L, A, At, s, B, P.PRECOND_JACOBI, X0=X0)
            for j, (x, info, st) in enumerate(alone):
                SV.assert_column((s.name, kernel, j), X[:, j], infos[j], cs[j], x, info, st)
    assert infos[2].iterations == 0 and infos[2].converged == 1 and M.same_bits(X[:, 2], X0[:, 2]).all()
    assert infos[0].iterations > infos[1].iterations > 0, [i.iterations for i in infos]


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_one_column_is_fs_pcg(L, mode):
    assert len(SV.PLAIN_SET) >= 20
    for name in SV.PLAIN_SET:
        s = SV.ALL[name]
        for precond in (P.PRECOND_NONE, P.PRECOND_JACOBI):
            with G.mode_options(mode):
                A, At = SV.handles(L, s)
                xp, ip, stp = SV.pcg_run(L, A, At, s, precond)
                X, infos, st, cs = SV.pcgn_run(L, A, At, s, s.b.reshape(-1, 1), precond)
            want = dict(stp)
            if ip.iterations == 0:
                want.pop("beta")                                    # (never written: whatever the allocation held)
            bad = M.mismatch(X[:, 0], xp, infos[0].iterations, ip.iterations, st, want)
            assert bad is None, f"fs_pcgn with k = 1 vs fs_pcg [{mode}] on {name}, precond {precond}: {bad}"
            assert infos[0].converged == ip.converged and M.same_bits(infos[0].rnorm, ip.rnorm)[0] and M.same_bits(infos[0].bnorm, ip.bnorm)[0]


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
_RECIPE8 = {}


def _recipe8(kind):
    if kind not in _RECIPE8:
        s, B, _ = N.recipe8(kind)
        _RECIPE8[kind] = (s, B, N.run(s, B, P.PRECOND_JACOBI))
    return _RECIPE8[kind]


@pytest.mark.parametrize("kind", list(N.KIND_ID))
def test_default_modes_eight_columns_within_the_bars(L, kind):
    s, B, model = _recipe8(kind)
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), s.t_csr_coo())
    assert all(i.converged == 1 for i in model.infos)
    for mode in ("default", "cg_fixed_order=0"):
        with G.mode_options(mode):
            A, At = SV.handles(L, s)
            runs = [SV.pcgn_run(L, A, At, s, B, P.PRECOND_JACOBI) for _ in range(2)]
        X, infos, _, _ = runs[0]
        for j in range(8):
            info = infos[j]
            nb = np.linalg.norm(B[:, j])
            res = float(np.linalg.norm(atm(am(X[:, j])) + s.lam * X[:, j] - B[:, j]) / nb) if nb else 0.0
            print(f"{s.name} [{mode}] column {j}: {info.iterations} iterations (model {model.infos[j].iterations}), true residual "
                  f"{res / s.tol:.2f} tol")
            what = (s.name, mode, j, info.iterations, model.infos[j].iterations, res)
            assert info.converged == 1, what
            assert res <= 2 * s.tol, what
            assert abs(info.iterations - model.infos[j].iterations) <= 1, what
            assert info.rnorm <= s.tol * info.bnorm, what
        assert infos[3].iterations == 0 and M.same_bits(X[:, 3], np.zeros(s.ncol)).all()
        if mode == "default":                                       # fixed-order products: a solve repeats its bits
            assert M.same_bits(runs[1][0], X).all() and [i.iterations for i in runs[1][1]] == [i.iterations for i in infos], (s.name, mode)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_a_nan_column_stays_in_its_column(L):
    s = SV.ALL["binary_F257"]
    B = SV.columns(s, 5)
    B[7, 3] = np.nan
    with G.options(strict_order=1):
        A, At = SV.handles(L, s)
        alone = {j: _pcg_column(L, A, At, s, B[:, j], P.PRECOND_JACOBI, max_iter=5) for j in (0, 1, 2, 4)}
        for kernel in SV.KERNELS:
            with G.options(pcgn_kernel=kernel):
                X, infos, st, cs = SV.pcgn_run(L, A, At, s, B, P.PRECOND_JACOBI, max_iter=5)
            assert infos[3].converged == 0 and infos[3].iterations == 5 and cs[3]["live"] == 1.0, (kernel, infos[3].iterations, infos[3].converged, cs[3])
            for j, (x, info, stj) in alone.items():
                SV.assert_column((s.name, kernel, j), X[:, j], infos[j], cs[j], x, info, stj)
                assert np.isfinite(X[:, j]).all()
            assert st["done"] == 0.0 and st["iter"] == 5.0


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_statuses(L):
    from libfastsparse_amd import capi
    s = SV.RECIPES["scaled_seed0"]
    A, At = SV.handles(L, s)
    st = capi.current_stream()
    k = 3
    B = G.to_device(SV.columns(s, k))
    X, d = G.nan_vector(s.ncol * N.MAX_RHS), G.to_device(SV.caller_diag(s))
    x_bits = X.cpu().numpy().view(np.int64).copy()

    def call(A_=A.h, At_=At.h, x_=X.data_ptr(), b_=B.data_ptr(), k_=k, prm="default", info=None, **kw):
        if prm == "default":
            f = dict(tol=1e-8, max_iter=0, precond=P.PRECOND_JACOBI, warm_start=0, diag=None)
            f.update(kw)
            prm = C.byref(capi.PcgParams(f["tol"], f["max_iter"], f["precond"], f["warm_start"], f["diag"]))
        return L.fs_pcgn(A_, At_, x_, b_, k_, s.lam, prm, info, st)

    bad = {"NULL A": call(A_=None), "NULL At": call(At_=None), "NULL X": call(x_=None), "NULL B": call(b_=None), "NULL prm": call(prm=None),
           "At of A's shape": call(At_=A.h), "k 0": call(k_=0), "k -1": call(k_=-1), "k 33": call(k_=33),
           "precond 3": call(precond=3), "precond -1": call(precond=-1), "DIAG without diag": call(precond=P.PRECOND_DIAG),
           "tol < 0": call(tol=-1e-8), "tol NaN": call(tol=float("nan")), "tol -inf": call(tol=float("-inf"))}
    assert all(rc == FS_ERR_ARG for rc in bad.values()), bad
    assert L.fs_last_error()
    SV.refused_call_leaves(X, x_bits)
    assert call(tol=0.0, max_iter=2) == FS_OK                        # tol = 0 is legal: the cap ends it; info NULL is legal too
    infos = (capi.PcgInfo * k)()
    assert call(tol=0.0, max_iter=2, info=infos) == FS_OK
    assert [i.iterations for i in infos] == [2, 2, 0] and [i.converged for i in infos] == [0, 0, 1]
    assert call(precond=P.PRECOND_NONE, diag=d.data_ptr(), max_iter=1) == FS_OK   # diag is ignored unless FS_PRECOND_DIAG


def test_released_handles(L):
    """FS_ERR_RELEASED before anything is written to X: Jacobi after fs_matrix_release_csr on a kept two-pass A'; a k that was never
    prepared before the release.  After fs_matrix_restore_csr the same bits return."""
    from libfastsparse_amd import capi
    s = SV.RECIPES["scaled_seed0"]
    st = capi.current_stream()
    trp, tcc, tvv = s.t_csr_coo()
    k = 3
    B = SV.columns(s, k)
    A, _ = SV.handles(L, s)
    with G.options(binning=2, bin_flags=64):                         # a kept two-pass copy: there is something to release for
        At = capi.Matrix.from_csr(s.ncol, s.nrow, G.to_device(trp), G.to_device(tcc), G.to_device(tvv))
    assert At.kernel_name() == "two-pass"
    X_before, infos_before, _, _ = SV.pcgn_run(L, A, At, s, B, P.PRECOND_JACOBI)          # prepares k = 3
    assert all(i.converged == 1 for i in infos_before)
    assert At.release_csr() == 1
    X = G.nan_vector(s.ncol * 4)
    bits = X.cpu().numpy().view(np.int64).copy()
    Bd, B4 = G.to_device(B), G.to_device(SV.columns(s, 4))
    jac, none = capi.PcgParams(s.tol, 0, P.PRECOND_JACOBI, 0, None), capi.PcgParams(s.tol, 3, P.PRECOND_NONE, 0, None)
    assert L.fs_pcgn(A.h, At.h, X.data_ptr(), Bd.data_ptr(), k, s.lam, C.byref(jac), None, st) == FS_ERR_RELEASED
    assert b"fs_matrix_release_csr" in L.fs_last_error()
    SV.refused_call_leaves(X, bits, "the refused Jacobi solve wrote to X")
    # k = 4 was never prepared on this A': fs_matrix_prepare needs the plain arrays
    assert L.fs_pcgn(A.h, At.h, X.data_ptr(), B4.data_ptr(), 4, s.lam, C.byref(none), None, st) == FS_ERR_RELEASED
    SV.refused_call_leaves(X, bits, "the refused k = 4 solve wrote to X")
    At.restore_csr(G.to_device(trp), G.to_device(tcc), G.to_device(tvv))
    X_after, infos_after, _, _ = SV.pcgn_run(L, A, At, s, B, P.PRECOND_JACOBI)
    assert [i.iterations for i in infos_after] == [i.iterations for i in infos_before] and M.same_bits(X_after, X_before).all()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_guard_zones(L):
    """X, B and diag inside guard zones (tests/_lifecycle.py), 16-byte aligned and 8 bytes off, both kernel variants: guards
    untouched, B and diag unchanged, and the result 8 bytes off has the bits of the aligned one"""
    import torch
    from libfastsparse_amd import capi
    mem = LC.TorchMem()
    st = capi.current_stream()
    for name in ("scaled_seed0", "binary_F257"):
        s = SV.ALL[name]
        A, At = SV.handles(L, s)
        diag = SV.caller_diag(s)
        n = s.ncol * 4
        gx, gb, gd = LC.Guarded(mem, "X of fs_pcgn", n), LC.Guarded(mem, "B of fs_pcgn", n), LC.Guarded(mem, "diag of fs_pcgn", s.ncol)
        for kernel, k in [(v, k) for v in SV.KERNELS for k in (3, 4)]:
            B = SV.columns(s, k)
            X0 = SV.x0_columns(s, B)
            for what, precond, warm, max_iter in SV.CASES:
                aligned = None
                for off in (0, 1):
                    mem.put(gb.place(s.ncol * k, off), B.reshape(-1))
                    mem.put(gd.place(s.ncol, off ^ 1), diag)
                    if warm:
                        mem.put(gx.place(s.ncol * k, off), X0.reshape(-1))
                    else:
                        mem.fill_bits(gx.place(s.ncol * k, off), LC.PREFILLS["nan"])
                    prm = capi.PcgParams(s.tol, max_iter, precond, int(warm), gd.view.data_ptr() if precond == P.PRECOND_DIAG else None)
                    infos = (capi.PcgInfo * k)()
                    with G.options(pcgn_kernel=kernel):
                        capi.check(L.fs_pcgn(A.h, At.h, gx.view.data_ptr(), gb.view.data_ptr(), k, s.lam, C.byref(prm), infos, st), "fs_pcgn")
                    torch.cuda.synchronize()
                    where = (name, kernel, k, what, off)
                    bad = mem.first_bad_guard([gx, gb, gd])
                    assert bad is None, (where, bad.first_broken())
                    assert mem.eq(gb.view, mem.const(B.reshape(-1))) and mem.eq(gd.view, mem.const(diag)), (where, "an input changed")
                    got = mem.get(gx.view)
                    assert np.isfinite(got).all(), where
                    if not max_iter and precond != P.PRECOND_NONE:
                        assert all(i.converged == 1 for i in infos), (where, [i.iterations for i in infos])
                    # the placement picks 16-byte or 8-byte accesses, never a bit (fixed-order products: a solve repeats its bits)
                    if aligned is None:
                        aligned = (got.copy(), [i.iterations for i in infos])
                    else:
                        assert M.same_bits(got, aligned[0]).all() and [i.iterations for i in infos] == aligned[1], (where, "differs from off = 0")


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_the_solve_prepares_the_k_column_products(L):
    from libfastsparse_amd import capi
    s = SV.RECIPES["powerlaw_seed0"]
    arp, acc, avv = s.a_csr()
    trp, tcc, tvv = s.t_csr_coo()
    # a matrix this small keeps and extends the two-pass copy only under binning = 2; the solver's own options are the defaults
    with G.options(binning=2, bin_flags=64):
        A = capi.Matrix.from_csr(s.nrow, s.ncol, G.to_device(arp), G.to_device(acc), None if avv is None else G.to_device(avv))
        At = capi.Matrix.from_csr(s.ncol, s.nrow, G.to_device(trp), G.to_device(tcc), None if tvv is None else G.to_device(tvv))
        assert A.kernel_name() == "two-pass" and At.kernel_name() == "two-pass"
        assert A.spmm_plan(4) != "k-column two-pass" and At.spmm_plan(4) != "k-column two-pass"
        B = SV.columns(s, 4)
        _, infos, _, _ = SV.pcgn_run(L, A, At, s, B, P.PRECOND_JACOBI)
        assert all(i.converged == 1 for i in infos)
        assert A.spmm_plan(4) == "k-column two-pass" and At.spmm_plan(4) == "k-column two-pass"
