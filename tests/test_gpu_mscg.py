"""fs_mscg against the CPU model of its device arithmetic (tests/_mscg_model.py), on the harness of tests/_solvers.py.

1  strict_order: X, every fs_pcg_info and the per-shift state have the model's bits -- one lambda, three with the minimum twice, the
   ladder of eight (shuffled) and sixteen; also under a cap of 5; also on more than one grid stride.
2  every mode: the columns of the smallest lambda are fs_cg at that lambda on the same handles, bit for bit, with the same count.
3  every mode: one lambda is fs_pcg with FS_PRECOND_NONE from a cold start at the same cap, bit for bit, info and b = 0 included.
4  default modes on the control / powerlaw recipes with the ladder of eight: every shift converged, true residual (the oracle's
   products) <= 2 tol, rnorm <= tol bnorm, within the error bound of a separate fs_pcg solve per lambda; fixed-order solves repeat
   their bits.
5  statuses: every FS_ERR_ARG leaves X untouched; tol = 0 with a cap and info = NULL are legal; a product's own error
   (FS_ERR_RELEASED under strict_order after fs_matrix_release_csr) is passed through.
6  guard zones around X (ldx = F and F + 3, 16-byte aligned and 8 bytes off) and b; the gaps between columns keep their bits."""
import ctypes as C

import numpy as np
import pytest

import _cg_model as M
import _gpu as G
import _lifecycle as LC
import _mscg_model as S
import _pcg_model as P
import _solvers as SV
from _gpu import FS_ERR_ARG, FS_ERR_RELEASED, FS_OK, L  # noqa: F401

pytestmark = pytest.mark.gpu

STRICT_SET = list(SV.DIAG_SET) + [n for n in SV.MSCG_RECIPES if n not in SV.DIAG_SET]
# factors on the system's own lambda (offsets where that is 0): one; three with the minimum twice; the ladder, shuffled; sixteen
STRICT_CASES = [(n, l, cap) for n in STRICT_SET for l in SV.LADDERS for cap in (0, 5)] + [("binary_F262145", "m8", 0), ("binary_F262145", "m3", 5)]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ladder,cap", STRICT_CASES, ids=[f"{n}-{l}-cap{c}" for n, l, c in STRICT_CASES])
def test_fs_mscg_strict_is_the_model(L, name, ladder, cap):
    s = SV.MSCG_ALL[name]
    lams = SV.lams_of(s, ladder)
    model = S.run(s, lams, max_iter=cap)
    with G.options(strict_order=1):
        A, At = SV.handles(L, s)
        X, infos, st, shifts = SV.mscg_run(L, A, At, s, lams, cap)
    what = f"fs_mscg {ladder} cap {cap} on {name}"
    print(f"{what}: counts {[i.iterations for i in infos]} (model {[i.iterations for i in model.infos]})")
    bad = M.mismatch(X, model.X, [i.iterations for i in infos], [i.iterations for i in model.infos], st, model.state)
    assert bad is None, f"{what}: {bad}"
    bad = S.shifts_mismatch(shifts, model.shifts)
    assert bad is None, f"{what}: {bad}"
    SV.assert_infos(what, infos, model.infos)
    if cap:
        assert all(i.iterations <= cap for i in infos)
    if name == "zero_rhs":
        assert all(i.converged == 1 and i.iterations == 0 for i in infos) and M.same_bits(X, np.zeros(X.shape)).all()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
BASE_SET = [n for n in STRICT_SET if np.any(SV.MSCG_ALL[n].b != 0)]


@pytest.mark.parametrize("name", BASE_SET)
@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_columns_of_the_smallest_lambda_are_fs_cg(L, mode, name):
    s = SV.MSCG_ALL[name]
    with G.mode_options(mode):
        A, At = SV.handles(L, s)
        xc, itc, stc = SV.fs_cg_on(L, A, At, s)
        for ladder in ("m3", "m8", "m16"):
            lams = SV.lams_of(s, ladder)
            X, infos, st, shifts = SV.mscg_run(L, A, At, s, lams)
            cols = [i for i, lam in enumerate(lams) if lam == min(lams)]
            assert min(lams) == s.lam and len(cols) == {"m3": 2, "m8": 1, "m16": 2}[ladder]
            want = {k: stc[k] for k in ("alpha", "beta", "stop", "rsq", "done", "iter")}
            if itc == 0:
                want.pop("beta")                                    # (never written: whatever the allocation held)
            for i in cols:
                bad = M.mismatch(X[i], xc, infos[i].iterations, itc, st, want)
                assert bad is None, f"column {i} of fs_mscg {ladder} vs fs_cg [{mode}] on {name}: {bad}"
                assert infos[i].converged == int(stc["done"]) and shifts["z"][i] == 1.0 and shifts["pslot"][i] == -1.0, (mode, name, i)


def test_the_base_set_is_whole():
    assert len(BASE_SET) >= 12


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", (0, 5))
@pytest.mark.parametrize("name", STRICT_SET)
@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_one_lambda_is_fs_pcg_without_preconditioner(L, mode, name, cap):
    s = SV.MSCG_ALL[name]
    with G.mode_options(mode):
        A, At = SV.handles(L, s)
        xp, ip, stp = SV.pcg_run(L, A, At, s, max_iter=cap)
        X, infos, st, _ = SV.mscg_run(L, A, At, s, [s.lam], cap)
    want = dict(stp)
    if stp["bb"] == 0.0:                                            # done before the first iteration: fs_pcg never writes these
        for k in ("rsq", "alpha", "beta"):
            want.pop(k)
    elif ip.iterations == 0:
        want.pop("beta")                                            # (never written by either)
    bad = M.mismatch(X[0], xp, infos[0].iterations, ip.iterations, st, want)
    assert bad is None, f"fs_mscg with one lambda vs fs_pcg [{mode}] cap {cap} on {name}: {bad}"
    SV.assert_infos((mode, name, cap), infos, [S.Info(ip.iterations, ip.converged, ip.rnorm, ip.bnorm)])
    if name == "zero_rhs":
        assert infos[0].converged == 1 and infos[0].iterations == 0 and M.same_bits(X, np.zeros(X.shape)).all()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SV.MSCG_RECIPES))
def test_default_modes_ladder_within_the_bars(L, name):
    from libfastsparse_amd import capi
    s = SV.MSCG_RECIPES[name]
    lams = SV.lams_of(s, "m8")
    bn = np.linalg.norm(s.b)
    for mode in ("default", "cg_fixed_order=0"):
        with G.mode_options(mode):
            A, At = SV.handles(L, s)
            runs = [SV.mscg_run(L, A, At, s, lams) for _ in range(2)]
            singles = []
            for lam in lams:
                x = G.nan_vector(s.ncol)
                info = capi.pcg(A, At, x, G.to_device(s.b), lam, s.tol, precond=P.PRECOND_NONE, stream=capi.current_stream())
                singles.append((x.cpu().numpy(), info))
        X, infos, _, _ = runs[0]
        res = [SV.residual(s, X[i], lam) for i, lam in enumerate(lams)]
        print(f"{name} [{mode}]: counts {[i.iterations for i in infos]}, separate fs_pcg {[i.iterations for _, i in singles]}, "
              f"true residuals / tol {[round(r / s.tol, 2) for r in res]}")
        for i, lam in enumerate(lams):
            what = (name, mode, i, lam, infos[i].iterations, res[i])
            assert infos[i].converged == 1, what
            assert res[i] <= 2 * s.tol, what
            assert infos[i].rnorm <= s.tol * infos[i].bnorm, what
            xs, si = singles[i]
            assert si.converged == 1, what
            assert np.linalg.norm(X[i] - xs) <= (res[i] + SV.residual(s, xs, lam)) * bn / lam * 1.01, what
        if mode == "default":                                       # fixed-order products: a solve repeats its bits
            assert M.same_bits(runs[1][0], X).all() and [i.iterations for i in runs[1][1]] == [i.iterations for i in infos], name


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_statuses(L):
    from libfastsparse_amd import capi
    s = SV.MSCG_RECIPES["control_seed0"]
    A, At = SV.handles(L, s)
    st = capi.current_stream()
    F, m = s.ncol, 3
    b, X = G.to_device(s.b), G.nan_vector(16 * F)
    bits = X.cpu().numpy().view(np.int64).copy()
    lams = [s.lam * 3, s.lam, s.lam * 10]

    def call(A_=A.h, At_=At.h, X_=X.data_ptr(), ldx=F, b_=b.data_ptr(), m_=m, lam="default", tol=1e-8, max_iter=0, info=None):
        if lam == "default":
            lam = lams + [1.0] * (max(m_, m) - m)
        arr = None if lam is None else (C.c_double * len(lam))(*lam)
        return L.fs_mscg(A_, At_, X_, ldx, b_, m_, arr, tol, max_iter, info, st)

    bad = {"NULL A": call(A_=None), "NULL At": call(At_=None), "NULL X": call(X_=None), "NULL b": call(b_=None), "NULL lambda": call(lam=None),
           "At of A's shape": call(At_=A.h), "m 0": call(m_=0), "m -1": call(m_=-1), "m 17": call(m_=17), "ldx < F": call(ldx=F - 1),
           "ldx 0": call(ldx=0), "tol < 0": call(tol=-1e-8), "tol NaN": call(tol=float("nan")), "tol -inf": call(tol=float("-inf")),
           "lambda NaN": call(lam=[1.0, float("nan"), 2.0]), "lambda inf": call(lam=[float("inf"), 1.0, 2.0]),
           "lambda -inf": call(lam=[1.0, 2.0, float("-inf")])}
    assert all(rc == FS_ERR_ARG for rc in bad.values()), bad
    assert L.fs_last_error()
    SV.refused_call_leaves(X, bits)
    assert call(tol=0.0, max_iter=2) == FS_OK                        # tol = 0 is legal: the cap ends it (info NULL is legal too)
    assert call(m_=16) == FS_OK
    infos = (capi.PcgInfo * m)()
    assert call(tol=0.0, max_iter=2, info=infos) == FS_OK
    assert [i.iterations for i in infos] == [2, 2, 2] and not any(i.converged for i in infos)
    assert call(lam=[-0.25, s.lam, 0.0], max_iter=3) == FS_OK       # a negative lambda is the caller's business


def test_a_product_error_is_passed_through(L):
    """fs_mscg hands a product's own status on: under strict_order a product reads the plain CSR, so after fs_matrix_release_csr on
    A' the solve ends with FS_ERR_RELEASED and the product's message; outside strict_order the kept copy serves and the solve is
    the one from before the release, and after fs_matrix_restore_csr the strict solve runs again"""
    from libfastsparse_amd import capi
    s = SV.MSCG_RECIPES["powerlaw_seed0"]
    st = capi.current_stream()
    trp, tcc, tvv = s.t_csr_coo()
    lams = SV.lams_of(s, "m3")
    A, _ = SV.handles(L, s)
    with G.options(binning=2, bin_flags=64):                         # a kept two-pass copy: there is something to release for
        At = capi.Matrix.from_csr(s.ncol, s.nrow, G.to_device(trp), G.to_device(tcc), None if tvv is None else G.to_device(tvv))
    assert At.kernel_name() == "two-pass"
    X_before, infos_before, _, _ = SV.mscg_run(L, A, At, s, lams)
    assert all(i.converged == 1 for i in infos_before)
    assert At.release_csr() == 1
    X = G.nan_vector(len(lams) * s.ncol)
    arr = (C.c_double * len(lams))(*lams)
    with G.options(strict_order=1):
        assert L.fs_mscg(A.h, At.h, X.data_ptr(), s.ncol, G.to_device(s.b).data_ptr(), len(lams), arr, s.tol, 0, None, st) == FS_ERR_RELEASED
        assert b"fs_matrix_release_csr" in L.fs_last_error()
    X_after, infos_after, _, _ = SV.mscg_run(L, A, At, s, lams)         # the kept copy needs no plain array
    assert M.same_bits(X_after, X_before).all() and [i.iterations for i in infos_after] == [i.iterations for i in infos_before]
    At.restore_csr(G.to_device(trp), G.to_device(tcc), None if tvv is None else G.to_device(tvv))
    with G.options(strict_order=1):
        X_strict, infos_strict, _, _ = SV.mscg_run(L, A, At, s, lams)
    assert all(i.converged == 1 for i in infos_strict) and np.isfinite(X_strict).all()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_guard_zones(L):
    """X and b inside guard zones (tests/_lifecycle.py), 16-byte aligned and 8 bytes off, columns packed and padded"""
    import torch
    from libfastsparse_amd import capi
    mem = LC.TorchMem()
    st = capi.current_stream()
    gap_bits = LC.PREFILLS["nan"]
    for name in ("control_seed0", "powerlaw_seed0", "binary_F257"):
        s = SV.MSCG_ALL[name]
        F = s.ncol
        A, At = SV.handles(L, s)
        gx, gb = LC.Guarded(mem, "X of fs_mscg", 16 * (F + 3)), LC.Guarded(mem, "b of fs_mscg", F)
        for ladder, cap in (("m1", 0), ("m3", 0), ("m8", 0), ("m8", 5), ("m16", 0)):
            lams = SV.lams_of(s, ladder)
            m = len(lams)
            ref = None
            for ldx in (F, F + 3):
                for off in (0, 1):
                    mem.put(gb.place(F, off ^ (ldx & 1)), s.b)
                    n = (m - 1) * ldx + F
                    mem.fill_bits(gx.place(n, off), gap_bits)
                    infos = (capi.PcgInfo * m)()
                    capi.check(L.fs_mscg(A.h, At.h, gx.view.data_ptr(), ldx, gb.view.data_ptr(), m, (C.c_double * m)(*lams), s.tol, cap,
                                         infos, st), "fs_mscg")
                    torch.cuda.synchronize()
                    what = (name, ladder, cap, ldx, off)
                    bad = mem.first_bad_guard([gx, gb])
                    assert bad is None, (what, bad.first_broken())
                    assert mem.eq(gb.view, mem.const(s.b)), (what, "b changed")
                    X, gaps = SV.split_rows_and_gaps(mem.get(gx.view), m, F, ldx)
                    assert (gaps.view(np.int64) == gap_bits).all(), (what, "a gap between columns was written")
                    assert np.isfinite(X).all(), what
                    if not cap:
                        assert all(i.converged == 1 for i in infos), (what, [i.iterations for i in infos])
                    if ref is None:
                        ref = X
                    assert M.same_bits(X, ref).all(), (what, "the solution depends on where X lies")
