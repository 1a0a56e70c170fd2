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
import contextlib
import ctypes as C

import numpy as np
import pytest

import _cg_model as M
import _lifecycle as LC
import _pcg_model as P

pytestmark = pytest.mark.gpu

FS_OK, FS_ERR_ARG, FS_ERR_RELEASED = 0, -2, -5
MODES = ("default", "cg_fixed_order=0", "reproducible", "strict_order")
SYSTEMS = M.systems()
RECIPES = {s.name: s for s in (P.recipe(k, seed) for k in ("scaled", "powerlaw", "control") for seed in (0, 1, 2))}
ALL = dict(SYSTEMS, **RECIPES)
# valued / pattern-only; lambda = 0 with an empty column; rows of A' of 72 (scaled) and 2500 (powerlaw) entries
DIAG_SET = ("fixture_100x50", "binary_F65", "binary_F257", "valued", "lambda0_empty_column", "zero_rhs", "three_eigenvalues",
            "scaled_seed0", "powerlaw_seed0", "control_seed0")
# the solves of test 2: (case, precond, warm start, max_iter)
CASES = [("none", P.PRECOND_NONE, False, 0), ("jacobi", P.PRECOND_JACOBI, False, 0), ("diag", P.PRECOND_DIAG, False, 0),
         ("jacobi-warm", P.PRECOND_JACOBI, True, 0), ("none-warm", P.PRECOND_NONE, True, 0), ("jacobi-cap5", P.PRECOND_JACOBI, False, 5),
         ("diag-warm-cap3", P.PRECOND_DIAG, True, 3)]
SOLVE_SET = [(n, c) for n in DIAG_SET for c in range(len(CASES))] + \
            [(n, 1) for n in ("scaled_seed1", "scaled_seed2", "powerlaw_seed1", "powerlaw_seed2", "control_seed1", "control_seed2")] + \
            [("binary_F262145", 1), ("binary_F262145", 3)]         # more than one grid stride in the two-sum update kernel


@pytest.fixture(scope="module")
def L():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from libfastsparse_amd import capi
    lib = capi.lib()
    lib.fs_debug_last_cg_state.argtypes = [C.c_void_p]
    return lib


@contextlib.contextmanager
def options(**kw):
    from libfastsparse_amd import capi
    lib = capi.lib()
    old = {k: lib.fs_get_option(k.encode()) for k in kw}
    assert all(v != FS_ERR_ARG for v in old.values()), old
    try:
        for k, v in kw.items():
            capi.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            capi.set_option(k, v)


def _mode(mode):
    if mode == "default":
        return options()
    if mode == "cg_fixed_order=0":
        return options(cg_fixed_order=0)
    return options(**{mode: 1})


def _d(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def handles(L, s):
    """A and A' from COO as HipDeviceBackend.cg and fs_cg_run of test_gpu_cg.py upload them (A' in the caller's entry order)"""
    from libfastsparse_amd import capi
    vals = None if s.vals is None else _d(s.vals)
    A = capi.Matrix.from_coo(s.nrow, s.ncol, _d(s.rows), _d(s.cols), vals)
    At = capi.Matrix.from_coo(s.ncol, s.nrow, _d(s.cols), _d(s.rows), vals)
    if L.fs_get_option(b"strict_order") == 1:
        assert A.kernel_name() == "stream" and At.kernel_name() == "stream", (A.kernel_name(), At.kernel_name())
    return A, At


def _raw_state(L):
    st = np.full(M.CG_STATE_DOUBLES, np.nan)
    assert L.fs_debug_last_cg_state(st.ctypes.data) == M.CG_STATE_DOUBLES
    return st


def pcg_run(L, A, At, s, precond=P.PRECOND_NONE, warm=None, max_iter=0, diag=None, tol=None, b=None):
    """fs_pcg through capi.pcg: x, fs_pcg_info, the final st[] by name"""
    from libfastsparse_amd import capi
    bd = _d(s.b if b is None else b)
    x = _nan(s.ncol) if warm is None else _d(warm)
    dd = None if diag is None else _d(diag)
    info = capi.pcg(A, At, x, bd, s.lam, s.tol if tol is None else tol, max_iter=max_iter, precond=precond, warm_start=warm is not None,
                    diag=dd, stream=capi.current_stream())
    return x.cpu().numpy(), info, P.state_from_device(_raw_state(L))


def fs_cg_on(L, A, At, s):
    from libfastsparse_amd import capi
    x, it = _nan(s.ncol), C.c_int(-1)
    capi.check(L.fs_cg(A.h, At.h, x.data_ptr(), _d(s.b).data_ptr(), s.lam, s.tol, C.byref(it), capi.current_stream()), "fs_cg")
    return x.cpu().numpy(), it.value, M.state_from_device(_raw_state(L), False)


def _caller_diag(s):
    """a positive diagonal that is not Jacobi's"""
    d = P.gram_diag(s.t_csr_coo(), s.lam)
    return np.abs(d) * (1.0 + 0.5 * np.cos(np.arange(s.ncol) * 1.7)) + 0.125


def _x0(s):
    return 0.5 * np.sin(np.arange(s.ncol) * 0.37 + 0.2) * np.linalg.norm(s.b) / max(1.0, np.sqrt(s.ncol))


def _assert_info(what, info, model):
    st = model.state
    assert info.iterations == model.iterations and info.converged == int(st["done"]), (what, info.iterations, info.converged, st)
    assert M.same_bits(info.rnorm, np.sqrt(st["rr"]))[0] and M.same_bits(info.bnorm, np.sqrt(st["bb"]))[0], (what, info.rnorm, info.bnorm, st)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DIAG_SET)
def test_gram_diag_strict_is_the_model(L, name):
    from libfastsparse_amd import capi
    s = ALL[name]
    t_csr = s.t_csr_coo()
    if name == "lambda0_empty_column":
        assert s.lam == 0.0 and np.diff(t_csr[0])[5] == 0
    if name in ("scaled_seed0", "powerlaw_seed0"):
        assert np.diff(t_csr[0]).max() > 64
    with options(strict_order=1):
        A, At = handles(L, s)
        for lam in (s.lam, 0.0, 0.75):
            d = _nan(s.ncol)
            capi.gram_diag(At, lam, d, capi.current_stream())
            got, want = d.cpu().numpy(), P.gram_diag(t_csr, lam)
            ok = M.same_bits(got, want)
            assert ok.all(), (name, lam, int((~ok).sum()), int(np.flatnonzero(~ok)[0]), got[~ok][:3], want[~ok][:3])
            if lam == 0.0 and name == "lambda0_empty_column":
                assert got[5] == 0.0 and not np.signbit(got[5])
    if s.vals is None:                                               # a pattern-only column: its count + lambda
        assert np.array_equal(P.gram_diag(t_csr, 0.0), np.diff(t_csr[0]).astype(float))


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case", SOLVE_SET, ids=[f"{n}-{CASES[c][0]}" for n, c in SOLVE_SET])
def test_fs_pcg_strict_is_the_model(L, name, case):
    s = ALL[name]
    what, precond, warm, max_iter = CASES[case]
    diag = _caller_diag(s) if precond == P.PRECOND_DIAG else None
    x0 = _x0(s) if warm else None
    model = P.run(s, precond, max_iter=max_iter, x0=x0, diag=diag)
    with options(strict_order=1):
        A, At = handles(L, s)
        x, info, st = pcg_run(L, A, At, s, precond, x0, max_iter, diag)
    bad = M.mismatch(x, model.x, info.iterations, model.iterations, st, model.state)
    assert bad is None, f"fs_pcg {what} on {name}: {bad}"
    _assert_info((name, what), info, model)
    if max_iter:
        assert info.iterations <= max_iter
    if name == "zero_rhs" and not warm:
        assert info.converged == 1 and info.iterations == 0 and M.same_bits(x, np.zeros(s.ncol)).all()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
PLAIN_SET = [n for n, s in ALL.items() if np.any(s.b != 0) and s.tol < 1]


@pytest.mark.parametrize("mode", MODES)
def test_without_preconditioner_cold_is_fs_cg(L, mode):
    assert len(PLAIN_SET) >= 20
    for name in PLAIN_SET:
        s = ALL[name]
        with _mode(mode):
            A, At = handles(L, s)
            xc, itc, stc = fs_cg_on(L, A, At, s)
            xp, info, stp = pcg_run(L, A, At, s)
        want = {k: stc[k] for k in ("alpha", "beta", "stop", "rsq", "done", "iter")}
        if itc == 0:
            want.pop("beta")                                        # (never written: whatever the allocation held)
        bad = M.mismatch(xp, xc, info.iterations, itc, stp, want)
        assert bad is None, f"fs_pcg without a preconditioner vs fs_cg [{mode}] on {name}: {bad}"
        assert info.converged == int(stc["done"]), (mode, name)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def _residual(s, x):
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), s.t_csr_coo())
    return float(np.linalg.norm(atm(am(x)) + s.lam * x - s.b) / np.linalg.norm(s.b))


@pytest.mark.parametrize("name", list(RECIPES))
def test_default_modes_jacobi_within_the_bars(L, name):
    s = RECIPES[name]
    model = P.run(s, P.PRECOND_JACOBI)
    assert model.state["done"] == 1.0
    for mode in ("default", "cg_fixed_order=0"):
        with _mode(mode):
            A, At = handles(L, s)
            runs = [pcg_run(L, A, At, s, P.PRECOND_JACOBI) for _ in range(2)]
            plain = pcg_run(L, A, At, s) if name.startswith("scaled") else None
        x, info, _ = runs[0]
        res = _residual(s, x)
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
                  f"true residual {_residual(s, plain[0]):.3g}")
            assert plain[1].converged == 0 and plain[1].iterations == s.ncol, (what, plain[1].iterations)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_statuses(L):
    from libfastsparse_amd import capi
    s = RECIPES["scaled_seed0"]
    A, At = handles(L, s)
    st = capi.current_stream()
    b, x, d = _d(s.b), _nan(s.ncol), _d(_caller_diag(s))
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
    assert np.array_equal(x.cpu().numpy().view(np.int64), x_bits), "a refused call wrote to x"
    assert call(tol=0.0, max_iter=2) == FS_OK                        # tol = 0 is legal: the cap ends it (info NULL is legal too)
    assert call(precond=P.PRECOND_NONE, diag=d.data_ptr(), max_iter=1) == FS_OK   # diag is ignored unless FS_PRECOND_DIAG


def test_released_transpose(L):
    """Jacobi reads the plain CSR of A'.  After fs_matrix_release_csr: FS_ERR_RELEASED before anything is written to x; a diagonal
    kept from before the release still serves FS_PRECOND_DIAG; after fs_matrix_restore_csr Jacobi is back, with the same bits (the
    same diagonal, fixed-order products)"""
    from libfastsparse_amd import capi
    s = RECIPES["scaled_seed0"]
    st = capi.current_stream()
    trp, tcc, tvv = s.t_csr_coo()
    A, _ = handles(L, s)
    with options(binning=2, bin_flags=64):                           # a kept two-pass copy: there is something to release for
        At = capi.Matrix.from_csr(s.ncol, s.nrow, _d(trp), _d(tcc), _d(tvv))
    assert At.kernel_name() == "two-pass"
    kept = _nan(s.ncol)
    capi.gram_diag(At, s.lam, kept, st)
    x_before, info_before, _ = pcg_run(L, A, At, s, P.PRECOND_JACOBI)
    assert info_before.converged == 1
    assert At.release_csr() == 1
    x = _nan(s.ncol)
    bits = x.cpu().numpy().view(np.int64).copy()
    prm = capi.PcgParams(s.tol, 0, P.PRECOND_JACOBI, 0, None)
    assert L.fs_pcg(A.h, At.h, x.data_ptr(), _d(s.b).data_ptr(), s.lam, C.byref(prm), None, st) == FS_ERR_RELEASED
    assert b"fs_matrix_release_csr" in L.fs_last_error()
    assert np.array_equal(x.cpu().numpy().view(np.int64), bits), "the refused solve wrote to x"
    assert L.fs_gram_diag(At.h, s.lam, x.data_ptr(), st) == FS_ERR_RELEASED
    assert np.array_equal(x.cpu().numpy().view(np.int64), bits), "the refused fs_gram_diag wrote to d"
    x_diag, info_diag, _ = pcg_run(L, A, At, s, P.PRECOND_DIAG, diag=kept.cpu().numpy())
    assert info_diag.converged == 1 and info_diag.iterations == info_before.iterations and M.same_bits(x_diag, x_before).all()
    x_none, info_none, _ = pcg_run(L, A, At, s, max_iter=3)          # no preconditioner: nothing reads the plain arrays either
    assert info_none.iterations == 3
    At.restore_csr(_d(trp), _d(tcc), _d(tvv))
    x_after, info_after, _ = pcg_run(L, A, At, s, P.PRECOND_JACOBI)
    assert info_after.converged == 1 and info_after.iterations == info_before.iterations and M.same_bits(x_after, x_before).all()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_guard_zones(L):
    """x, b and diag inside guard zones (tests/_lifecycle.py), 16-byte aligned and 8 bytes off: guards untouched, b and diag unchanged"""
    import torch
    from libfastsparse_amd import capi
    mem = LC.TorchMem()
    st = capi.current_stream()
    for name in ("scaled_seed0", "powerlaw_seed0", "binary_F257"):
        s = ALL[name]
        A, At = handles(L, s)
        diag = _caller_diag(s)
        gx, gb, gd = LC.Guarded(mem, "x of fs_pcg", s.ncol), LC.Guarded(mem, "b of fs_pcg", s.ncol), LC.Guarded(mem, "diag of fs_pcg", s.ncol)
        for off in (0, 1):
            for what, precond, warm, max_iter in CASES:
                mem.put(gb.place(s.ncol, off), s.b)
                mem.put(gd.place(s.ncol, off ^ 1), diag)
                if warm:
                    mem.put(gx.place(s.ncol, off), _x0(s))
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
