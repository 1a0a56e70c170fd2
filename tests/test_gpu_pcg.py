"""fs_gram_diag and fs_pcg against the CPU model of their device arithmetic (tests/_pcg_model.py).

1  strict_order: fs_gram_diag has the model's bits -- valued and pattern-only, an empty column with lambda = 0, rows of A' longer
   than one wave.
2  strict_order: fs_pcg has the model's bits in x, the count, the state and fs_pcg_info -- no preconditioner, Jacobi, a caller's
   diagonal, warm starts, an iteration cap.
3  every mode: without a preconditioner, from a cold start, fs_pcg IS fs_cg on the same handles, bit for bit (the same kernels on
   the same data: no tolerance).
4  default modes on the systems a diagonal preconditioner is for: Jacobi converges, true residual (the oracle's products) <= 2 tol,
   the count within one of the model's (preconditioned cond 4.6: the bar of well-conditioned systems); fixed-order solves repeat
   their bits; plain CG on the column-scaled system ends at the cap, not converged.
5  statuses: every FS_ERR_ARG, FS_ERR_RELEASED for Jacobi after fs_matrix_release_csr (x untouched; a kept diagonal still works;
   Jacobi again after fs_matrix_restore_csr).
6  guard zones around x, b and diag."""
import ctypes as C

import numpy as np
import pytest

import _cg_model as M
import _gpu as G
import _lifecycle as LC
import _pcg_model as P
import _solvers as SV
from _gpu import FS_ERR_ARG, FS_ERR_RELEASED, FS_OK, L  # noqa: F401

pytestmark = pytest.mark.gpu

# the solves of test 2: every case of SV.CASES on SV.DIAG_SET, Jacobi on the other seeds
SOLVE_SET = [(n, c) for n in SV.DIAG_SET for c in range(len(SV.CASES))] + \
            [(n, 1) for n in ("scaled_seed1", "scaled_seed2", "powerlaw_seed1", "powerlaw_seed2", "control_seed1", "control_seed2")] + \
            [("binary_F262145", 1), ("binary_F262145", 3)]         # more than one grid stride in the two-sum update kernel


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SV.DIAG_SET)
def test_gram_diag_strict_is_the_model(L, name):
    from libfastsparse_amd import capi
    s = SV.ALL[name]
    t_csr = s.t_csr_coo()
    if name == "lambda0_empty_column":
        assert s.lam == 0.0 and np.diff(t_csr[0])[5] == 0
    if name in ("scaled_seed0", "powerlaw_seed0"):
        assert np.diff(t_csr[0]).max() > 64
    with G.options(strict_order=1):
        A, At = SV.handles(L, s)
        for lam in (s.lam, 0.0, 0.75):
            d = G.nan_vector(s.ncol)
            capi.gram_diag(At, lam, d, capi.current_stream())
            got, want = d.cpu().numpy(), P.gram_diag(t_csr, lam)
            ok = M.same_bits(got, want)
            assert ok.all(), (name, lam, int((~ok).sum()), int(np.flatnonzero(~ok)[0]), got[~ok][:3], want[~ok][:3])
            if lam == 0.0 and name == "lambda0_empty_column":
                assert got[5] == 0.0 and not np.signbit(got[5])
    if s.vals is None:                                               # a pattern-only column: its count + lambda
        assert np.array_equal(P.gram_diag(t_csr, 0.0), np.diff(t_csr[0]).astype(float))


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case", SOLVE_SET, ids=[f"{n}-{SV.CASES[c][0]}" for n, c in SOLVE_SET])
def test_fs_pcg_strict_is_the_model(L, name, case):
    s = SV.ALL[name]
    what, precond, warm, max_iter = SV.CASES[case]
    diag = SV.caller_diag(s) if precond == P.PRECOND_DIAG else None
    x0 = SV.x0(s) if warm else None
    model = P.run(s, precond, max_iter=max_iter, x0=x0, diag=diag)
    with G.options(strict_order=1):
        A, At = SV.handles(L, s)
        x, info, st = SV.pcg_run(L, A, At, s, precond, x0, max_iter, diag)
    bad = M.mismatch(x, model.x, info.iterations, model.iterations, st, model.state)
    assert bad is None, f"fs_pcg {what} on {name}: {bad}"
    SV.assert_info((name, what), info, model)
    if max_iter:
        assert info.iterations <= max_iter
    if name == "zero_rhs" and not warm:
        assert info.converged == 1 and info.iterations == 0 and M.same_bits(x, np.zeros(s.ncol)).all()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_without_preconditioner_cold_is_fs_cg(L, mode):
    assert len(SV.PLAIN_SET) >= 20
    for name in SV.PLAIN_SET:
        s = SV.ALL[name]
        with G.mode_options(mode):
            A, At = SV.handles(L, s)
            xc, itc, stc = SV.fs_cg_on(L, A, At, s)
            xp, info, stp = SV.pcg_run(L, A, At, s)
        want = {k: stc[k] for k in ("alpha", "beta", "stop", "rsq", "done", "iter")}
        if itc == 0:
            want.pop("beta")                                        # (never written: whatever the allocation held)
        bad = M.mismatch(xp, xc, info.iterations, itc, stp, want)
        assert bad is None, f"fs_pcg without a preconditioner vs fs_cg [{mode}] on {name}: {bad}"
        assert info.converged == int(stc["done"]), (mode, name)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SV.RECIPES))
def test_default_modes_jacobi_within_the_bars(L, name):
    s = SV.RECIPES[name]
    model = P.run(s, P.PRECOND_JACOBI)
    assert model.state["done"] == 1.0
    for mode in ("default", "cg_fixed_order=0"):
        with G.mode_options(mode):
            A, At = SV.handles(L, s)
            runs = [SV.pcg_run(L, A, At, s, P.PRECOND_JACOBI) for _ in range(2)]
            plain = SV.pcg_run(L, A, At, s) if name.startswith("scaled") else None
        x, info, _ = runs[0]
        res = SV.residual(s, x)
        print(f"{name} [{mode}]: jacobi {info.iterations} iterations (model {model.iterations}), true residual {res:.3g} "
              f"= {res / s.tol:.2f} tol, rnorm / bnorm {info.rnorm / info.bnorm:.3g}")
        what = (name, mode, info.iterations, model.iterations, res)
        assert info.converged == 1, what
        assert res <= 2 * s.tol, what
        assert abs(info.iterations - model.iterations) <= 1, what
        assert info.rnorm <= s.tol * info.bnorm, what
        if mode == "default":                                       # fixed-order products: a solve repeats its bits
            assert runs[1][1].iterations == info.iterations and M.same_bits(runs[1][0], x).all(), what
        if plain is not None:
            print(f"{name} [{mode}]: plain {plain[1].iterations} iterations, converged {plain[1].converged}, "
                  f"true residual {SV.residual(s, plain[0]):.3g}")
            assert plain[1].converged == 0 and plain[1].iterations == s.ncol, (what, plain[1].iterations)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_statuses(L):
    from libfastsparse_amd import capi
    s = SV.RECIPES["scaled_seed0"]
    A, At = SV.handles(L, s)
    st = capi.current_stream()
    b, x, d = G.to_device(s.b), G.nan_vector(s.ncol), G.to_device(SV.caller_diag(s))
    x_bits = x.cpu().numpy().view(np.int64).copy()

    def call(A_=A.h, At_=At.h, x_=x.data_ptr(), b_=b.data_ptr(), prm="default", **kw):
        if prm == "default":
            f = dict(tol=1e-8, max_iter=0, precond=P.PRECOND_JACOBI, warm_start=0, diag=None)
            f.update(kw)
            prm = C.byref(capi.PcgParams(f["tol"], f["max_iter"], f["precond"], f["warm_start"], f["diag"]))
        return L.fs_pcg(A_, At_, x_, b_, s.lam, prm, None, st)

    bad = {"NULL A": call(A_=None), "NULL At": call(At_=None), "NULL x": call(x_=None), "NULL b": call(b_=None), "NULL prm": call(prm=None),
           "At of A's shape": call(At_=A.h), "precond 3": call(precond=3), "precond -1": call(precond=-1),
           "DIAG without diag": call(precond=P.PRECOND_DIAG), "tol < 0": call(tol=-1e-8), "tol NaN": call(tol=float("nan")),
           "tol -inf": call(tol=float("-inf"))}
    assert all(rc == FS_ERR_ARG for rc in bad.values()), bad
    assert L.fs_last_error()
    assert L.fs_gram_diag(None, 0.0, x.data_ptr(), st) == FS_ERR_ARG and L.fs_gram_diag(At.h, 0.0, None, st) == FS_ERR_ARG
    SV.refused_call_leaves(x, x_bits, "a refused call wrote to x")
    assert call(tol=0.0, max_iter=2) == FS_OK                        # tol = 0 is legal: the cap ends it (info NULL is legal too)
    assert call(precond=P.PRECOND_NONE, diag=d.data_ptr(), max_iter=1) == FS_OK   # diag is ignored unless FS_PRECOND_DIAG


def test_released_transpose(L):
    """Jacobi reads the plain CSR of A'.  After fs_matrix_release_csr: FS_ERR_RELEASED before anything is written to x; a diagonal
    kept from before the release still serves FS_PRECOND_DIAG; after fs_matrix_restore_csr Jacobi is back, with the same bits (the
    same diagonal, fixed-order products)"""
    from libfastsparse_amd import capi
    s = SV.RECIPES["scaled_seed0"]
    st = capi.current_stream()
    trp, tcc, tvv = s.t_csr_coo()
    A, _ = SV.handles(L, s)
    with G.options(binning=2, bin_flags=64):                           # a kept two-pass copy: there is something to release for
        At = capi.Matrix.from_csr(s.ncol, s.nrow, G.to_device(trp), G.to_device(tcc), G.to_device(tvv))
    assert At.kernel_name() == "two-pass"
    kept = G.nan_vector(s.ncol)
    capi.gram_diag(At, s.lam, kept, st)
    x_before, info_before, _ = SV.pcg_run(L, A, At, s, P.PRECOND_JACOBI)
    assert info_before.converged == 1
    assert At.release_csr() == 1
    x = G.nan_vector(s.ncol)
    bits = x.cpu().numpy().view(np.int64).copy()
    prm = capi.PcgParams(s.tol, 0, P.PRECOND_JACOBI, 0, None)
    assert L.fs_pcg(A.h, At.h, x.data_ptr(), G.to_device(s.b).data_ptr(), s.lam, C.byref(prm), None, st) == FS_ERR_RELEASED
    assert b"fs_matrix_release_csr" in L.fs_last_error()
    SV.refused_call_leaves(x, bits, "the refused solve wrote to x")
    assert L.fs_gram_diag(At.h, s.lam, x.data_ptr(), st) == FS_ERR_RELEASED
    SV.refused_call_leaves(x, bits, "the refused fs_gram_diag wrote to d")
    x_diag, info_diag, _ = SV.pcg_run(L, A, At, s, P.PRECOND_DIAG, diag=kept.cpu().numpy())
    assert info_diag.converged == 1 and info_diag.iterations == info_before.iterations and M.same_bits(x_diag, x_before).all()
    x_none, info_none, _ = SV.pcg_run(L, A, At, s, max_iter=3)          # no preconditioner: nothing reads the plain arrays either
    assert info_none.iterations == 3
    At.restore_csr(G.to_device(trp), G.to_device(tcc), G.to_device(tvv))
    x_after, info_after, _ = SV.pcg_run(L, A, At, s, P.PRECOND_JACOBI)
    assert info_after.converged == 1 and info_after.iterations == info_before.iterations and M.same_bits(x_after, x_before).all()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_guard_zones(L):
    """x, b and diag inside guard zones (tests/_lifecycle.py), 16-byte aligned and 8 bytes off: guards untouched, b and diag unchanged"""
    import torch
    from libfastsparse_amd import capi
    mem = LC.TorchMem()
    st = capi.current_stream()
    for name in ("scaled_seed0", "powerlaw_seed0", "binary_F257"):
        s = SV.ALL[name]
        A, At = SV.handles(L, s)
        diag = SV.caller_diag(s)
        gx, gb, gd = LC.Guarded(mem, "x of fs_pcg", s.ncol), LC.Guarded(mem, "b of fs_pcg", s.ncol), LC.Guarded(mem, "diag of fs_pcg", s.ncol)
        for off in (0, 1):
            for what, precond, warm, max_iter in SV.CASES:
                mem.put(gb.place(s.ncol, off), s.b)
                mem.put(gd.place(s.ncol, off ^ 1), diag)
                if warm:
                    mem.put(gx.place(s.ncol, off), SV.x0(s))
                else:
                    mem.fill_bits(gx.place(s.ncol, off), LC.PREFILLS["nan"])
                prm = capi.PcgParams(s.tol, max_iter, precond, int(warm), gd.view.data_ptr() if precond == P.PRECOND_DIAG else None)
                info = capi.PcgInfo()
                capi.check(L.fs_pcg(A.h, At.h, gx.view.data_ptr(), gb.view.data_ptr(), s.lam, C.byref(prm), C.byref(info), st), "fs_pcg")
                torch.cuda.synchronize()
                bad = mem.first_bad_guard([gx, gb, gd])
                assert bad is None, (name, what, off, bad.first_broken())
                assert mem.eq(gb.view, mem.const(s.b)) and mem.eq(gd.view, mem.const(diag)), (name, what, off, "an input changed")
                got = mem.get(gx.view)
                assert np.isfinite(got).all(), (name, what, off)
                if not max_iter and precond != P.PRECOND_NONE:
                    assert info.converged == 1, (name, what, off, info.iterations)
        gdiag = LC.Guarded(mem, "d of fs_gram_diag", s.ncol)
        for off in (0, 1):
            mem.fill_bits(gdiag.place(s.ncol, off), LC.PREFILLS["nan"])
            capi.gram_diag(At, s.lam, gdiag.view, st)
            torch.cuda.synchronize()
            assert gdiag.guards_ok(), (name, off, gdiag.first_broken())
            assert M.same_bits(mem.get(gdiag.view), P.gram_diag(s.t_csr_coo(), s.lam)).all(), (name, off)
