"""What the single-device solver suites share: the system tables, the runners of every solver entry point, the input makers, the
state readers and the assert helpers (tests/test_gpu_{cg,pcg,pcgn,pcgn_lambdas,pcgn_compact,mscg,mscgn}.py; the sharded half is
tests/_dist_solvers.py).  The device basics are tests/_gpu.py.

torch and libfastsparse_amd are imported inside the functions: the module itself imports on a machine without a GPU."""
import ctypes as C
import os

import numpy as np

import _cg_model as M
import _lifecycle as LC
import _mscg_model as S
import _pcg_model as P
import _pcgn_lambdas_model as NL
import _pcgn_model as N
from _gpu import nan_vector, to_device, to_numpy

# ---- the systems -----------------------------------------------------------------------------------------------------------
ROW_PLAN = 1                                             # fs_matrix_spmm_plan code of the row kernel (storage-order sums)
SYSTEMS = M.systems()
DIST_SET = ("fixture_100x50", "binary_F65", "binary_F262145", "ill_conditioned", "cap_tol0", "three_eigenvalues", "zero_rhs",
            "cg2_equal_columns", "lambda0_empty_column", "valued")
RECIPES = {s.name: s for s in (P.recipe(k, seed) for k in ("scaled", "powerlaw", "control") for seed in (0, 1, 2))}
ALL = dict(SYSTEMS, **RECIPES)
# valued / pattern-only; lambda = 0 with an empty column; rows of A' of 72 (scaled) and 2500 (powerlaw) entries
DIAG_SET = ("fixture_100x50", "binary_F65", "binary_F257", "valued", "lambda0_empty_column", "zero_rhs", "three_eigenvalues",
            "scaled_seed0", "powerlaw_seed0", "control_seed0")
# the solves of fs_pcg: (case, precond, warm start, max_iter)
CASES = [("none", P.PRECOND_NONE, False, 0), ("jacobi", P.PRECOND_JACOBI, False, 0), ("diag", P.PRECOND_DIAG, False, 0),
         ("jacobi-warm", P.PRECOND_JACOBI, True, 0), ("none-warm", P.PRECOND_NONE, True, 0), ("jacobi-cap5", P.PRECOND_JACOBI, False, 5),
         ("diag-warm-cap3", P.PRECOND_DIAG, True, 3)]
PLAIN_SET = [n for n, s in ALL.items() if np.any(s.b != 0) and s.tol < 1]
EXACT = [(M.exact_system(), 4.0), (M.exact_system(m=7, lam=9.0, F=700, seed=17), 16.0), (M.exact_system(lam=0.5, nrow=0), 0.5)]
KS = (1, 2, 3, 4, 5, 7, 8, 16, 17, 32)
KERNELS = (1, 2)                                     # option "pcgn_kernel": a lane per row; the panels staged through LDS (0: auto)
# the systems of the ladder suites: fs_mscg's recipes, and every system with them
MSCG_RECIPES = {s.name: s for s in (P.recipe(k, seed) for k in ("control", "powerlaw") for seed in (0, 1, 2))}
MSCG_ALL = dict(ALL, **MSCG_RECIPES)
SHUFFLE8 = (5, 2, 7, 0, 3, 6, 1, 4)
# factors on the system's own lambda (offsets where that is 0): one; three with the minimum twice; the ladder, shuffled; sixteen
LADDERS = {"m1": (1.0,), "m3": (3.0, 1.0, 1.0), "m8": tuple(S.LADDER[k] for k in SHUFFLE8),
           "m16": tuple(float(f) for f in (7, 1, 2, 1e5, 3, 50, 1, 20, 1e3, 4, 300, 1e7, 5, 3, 12, 1.5))}


def lams_of(s, ladder):
    return [s.lam * f if s.lam else (f - 1.0) * 0.125 for f in LADDERS[ladder]]


# ---- the state readers -----------------------------------------------------------------------------------------------------
def cg_state(L, two):
    L.fs_debug_last_cg_state.argtypes = [C.c_void_p]
    st = np.full(M.CG_STATE_DOUBLES, np.nan)
    assert L.fs_debug_last_cg_state(st.ctypes.data) == M.CG_STATE_DOUBLES
    return M.state_from_device(st, two)


def raw_state(L):
    st = np.full(M.CG_STATE_DOUBLES, np.nan)
    assert L.fs_debug_last_cg_state(st.ctypes.data) == M.CG_STATE_DOUBLES
    return st


# ---- the input makers ------------------------------------------------------------------------------------------------------
def caller_diag(s):
    """a positive diagonal that is not Jacobi's"""
    d = P.gram_diag(s.t_csr_coo(), s.lam)
    return np.abs(d) * (1.0 + 0.5 * np.cos(np.arange(s.ncol) * 1.7)) + 0.125


def x0(s):
    return 0.5 * np.sin(np.arange(s.ncol) * 0.37 + 0.2) * np.linalg.norm(s.b) / max(1.0, np.sqrt(s.ncol))


def columns(s, k):
    """B (F, k): column 0 the system's b; from k >= 2 column 1 its bit-identical duplicate; from k >= 3 column 2 zero; the others
    deterministic and distinct"""
    i = np.arange(s.ncol, dtype=np.float64)
    B = np.empty((s.ncol, k))
    for j in range(k):
        B[:, j] = s.b * (1.0 + 0.25 * j) + np.sin(i * (0.11 * j) + 0.3 * j) * (0.5 + 0.125 * j)
    B[:, 0] = s.b
    if k >= 2:
        B[:, 1] = s.b
    if k >= 3:
        B[:, 2] = 0.0
    return B


def x0_columns(s, B):
    """a warm start per column, in the scale of that column (a zero column starts from +0.0)"""
    i = np.arange(s.ncol, dtype=np.float64)
    X0 = np.zeros(B.shape)
    for j in range(B.shape[1]):
        nb = np.linalg.norm(B[:, j])
        if nb:
            X0[:, j] = 0.5 * np.sin(i * 0.37 + 0.2 + (0.0 if j < 2 else j)) * nb / max(1.0, np.sqrt(s.ncol))
    return X0


def nonzero_columns(B):
    return [j for j in range(B.shape[1]) if B[:, j].any()]


_LADDERS = {}


def ladder(name):
    """the recipe's 8 rungs, B = b in every column, and the model's Jacobi solves (computed once, shared by the tests that run it)"""
    if name not in _LADDERS:
        s = RECIPES[name]
        lams = NL.rungs(s, 8)
        B = np.ascontiguousarray(np.repeat(s.b[:, None], 8, 1))
        _LADDERS[name] = (s, lams, B, NL.run(s, B, lams, P.PRECOND_JACOBI))
    return _LADDERS[name]


# ---- X with gaps between its rows ------------------------------------------------------------------------------------------
GAP_BITS = LC.PREFILLS["nan"]                                        # what the gaps are filled with


def strided_rows(m, F, ldx, hbm, fill_bits):
    """m rows of shape F (an int; (F, k) for panels) that begin ldx doubles apart in one buffer of (m - 1) ldx + size(F) doubles, host
    memory or HBM, every double prefilled with fill_bits: the buffer and the (m, *F) view of it"""
    shape = (F,) if isinstance(F, int) else tuple(F)
    n = (m - 1) * ldx + int(np.prod(shape))
    strides = (ldx,) + tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))
    if hbm:
        import torch
        buf = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
        buf.view(torch.int64).fill_(fill_bits)
        return buf, buf.as_strided((m,) + shape, strides)
    buf = np.full(max(n, 1), fill_bits, np.int64).view(np.float64)
    return buf, np.lib.stride_tricks.as_strided(buf, (m,) + shape, tuple(8 * v for v in strides))


def split_rows_and_gaps(buf, m, F, ldx):
    """the m rows of F doubles (m, F) and the doubles between them, laid end to end, of a buffer like strided_rows'"""
    got = to_numpy(buf)
    gaps = np.concatenate([got[i * ldx + F:(i + 1) * ldx] for i in range(m - 1)] + [np.zeros(0)])
    return np.stack([got[i * ldx:i * ldx + F] for i in range(m)]), gaps


def refused_call_leaves(X, bits, what="a refused call wrote to X"):
    assert np.array_equal(to_numpy(X).view(np.int64), bits), what


# ---- the entry points ------------------------------------------------------------------------------------------------------
def handles(L, s):
    """A and A' from COO as HipDeviceBackend.cg uploads them (A' in the caller's entry order)"""
    from libfastsparse_amd import capi
    vals = None if s.vals is None else to_device(s.vals)
    A = capi.Matrix.from_coo(s.nrow, s.ncol, to_device(s.rows), to_device(s.cols), vals)
    At = capi.Matrix.from_coo(s.ncol, s.nrow, to_device(s.cols), to_device(s.rows), vals)
    if L.fs_get_option(b"strict_order") == 1:
        assert A.kernel_name() == "stream" and At.kernel_name() == "stream", (A.kernel_name(), At.kernel_name())
    return A, At


def single_handles(L, s):
    """A from its CSR and the sorted A', as the shards of a built transpose hold them, on one device"""
    from libfastsparse_amd import capi
    (arp, acc, avv), (trp, tcc, tvv) = s.a_csr(), s.t_csr_sorted()
    A = capi.Matrix.from_csr(s.nrow, s.ncol, to_device(arp), to_device(acc), None if avv is None else to_device(avv))
    At = capi.Matrix.from_csr(s.ncol, s.nrow, to_device(trp), to_device(tcc), None if tvv is None else to_device(tvv))
    return A, At


def fs_cg_run(L, s, two, t_sorted=False, b=None):
    """fs_cg / fs_cg2 on handles: from COO like HipDeviceBackend.cg (A' in the caller's entry order), or (t_sorted) from the CSR
    of A and the A' of fs_dist_matrix_build_transpose, as fs_dist_cg holds them.  Returns x, the count, the final st[]."""
    import torch
    from libfastsparse_amd import capi
    A, At = single_handles(L, s) if t_sorted else handles(L, s)
    if L.fs_get_option(b"strict_order") == 1:
        assert A.kernel_name() == "stream" and At.kernel_name() == "stream", (A.kernel_name(), At.kernel_name())
    rhs = (s.B if two else s.b) if b is None else b
    bd = to_device(rhs.reshape(-1))
    x = torch.full((rhs.size,), float("nan"), dtype=torch.float64, device="cuda")
    it = C.c_int(-1)
    L.fs_debug_last_spmm_plan()
    f = L.fs_cg2 if two else L.fs_cg
    capi.check(f(A.h, At.h, x.data_ptr(), bd.data_ptr(), s.lam, s.tol, C.byref(it), capi.current_stream()), "fs_cg")
    if two and L.fs_get_option(b"strict_order") == 1:
        assert L.fs_debug_last_spmm_plan() == ROW_PLAN
    out = x.cpu().numpy()
    return (out.reshape(-1, 2) if two else out), it.value, cg_state(L, two)


def fs_cg_on(L, A, At, s):
    from libfastsparse_amd import capi
    x, it = nan_vector(s.ncol), C.c_int(-1)
    capi.check(L.fs_cg(A.h, At.h, x.data_ptr(), to_device(s.b).data_ptr(), s.lam, s.tol, C.byref(it), capi.current_stream()), "fs_cg")
    return x.cpu().numpy(), it.value, M.state_from_device(raw_state(L), False)


def dropin_run(L, s, two, b=None):
    """bsbm_cg / bsbm_cg2 on host structs (new_bsbm(A, 8), new_bsbm(A', 8)) and host vectors; also the CSR of A and A' the
    library uploads (the blocks laid end to end)"""
    import _hipbackend as H
    from oracle import pyoracle as O
    be = H.HipDropinBackend()
    st_a, st_t = be.sbm(s.nrow, s.ncol, s.rows, s.cols), be.sbm(s.ncol, s.nrow, s.cols, s.rows)
    Bl, Blt = L.new_bsbm(C.byref(st_a), 8), L.new_bsbm(C.byref(st_t), 8)

    def csr(Bp, nrow):
        B = Bp.contents
        n = [B.nnz[i] for i in range(B.nblocks)]
        rows = np.concatenate([np.ctypeslib.as_array(B.rows[i], shape=(k,)) for i, k in enumerate(n) if k] + [np.zeros(0, np.int32)])
        cols = np.concatenate([np.ctypeslib.as_array(B.cols[i], shape=(k,)) for i, k in enumerate(n) if k] + [np.zeros(0, np.int32)])
        return O.coo_to_csr(nrow, rows.astype(np.int32), cols.astype(np.int32), None)

    held = (csr(Bl, s.nrow), csr(Blt, s.ncol))
    rhs = np.ascontiguousarray((s.B if two else s.b) if b is None else b, dtype=np.float64).reshape(-1).copy()
    x = np.full(rhs.size, np.nan)
    it = C.c_int(-1)
    f = L.bsbm_cg2 if two else L.bsbm_cg
    f.restype = None
    L.fs_debug_last_spmm_plan()
    f(H._dp(x), Bl, Blt, H._dp(rhs), C.c_double(s.lam), C.c_double(s.tol), C.byref(it))
    if two and L.fs_get_option(b"strict_order") == 1 and os.environ.get("FASTSPARSE_NGPU", "1") in ("", "0", "1"):
        assert L.fs_debug_last_spmm_plan() == ROW_PLAN
    state = cg_state(L, two)
    L.fs_invalidate(Bl)
    L.fs_invalidate(Blt)
    return (x.reshape(-1, 2) if two else x), it.value, state, held


def pcg_run(L, A, At, s, precond=P.PRECOND_NONE, warm=None, max_iter=0, diag=None, tol=None, b=None):
    """fs_pcg through capi.pcg: x, fs_pcg_info, the final st[] by name"""
    from libfastsparse_amd import capi
    bd = to_device(s.b if b is None else b)
    x = nan_vector(s.ncol) if warm is None else to_device(warm)
    dd = None if diag is None else to_device(diag)
    info = capi.pcg(A, At, x, bd, s.lam, s.tol if tol is None else tol, max_iter=max_iter, precond=precond, warm_start=warm is not None,
                    diag=dd, stream=capi.current_stream())
    return x.cpu().numpy(), info, P.state_from_device(raw_state(L))


def pcgn_run(L, A, At, s, B, precond=P.PRECOND_NONE, X0=None, max_iter=0, diag=None, tol=None):
    """fs_pcgn through capi.pcgn: X (F, k), the infos, st[] by name, the per-column scalars by name"""
    from libfastsparse_amd import capi
    k = B.shape[1]
    Bd = to_device(B)
    X = nan_vector(s.ncol * k).view(s.ncol, k) if X0 is None else to_device(X0)
    dd = None if diag is None else to_device(diag)
    infos = capi.pcgn(A, At, X, Bd, s.lam, s.tol if tol is None else tol, max_iter=max_iter, precond=precond, warm_start=X0 is not None,
                      diag=dd, stream=capi.current_stream())
    raw = np.full(N.MAX_RHS * N.PN_STRIDE, np.nan)
    assert L.fs_debug_last_pcgn_state(raw.ctypes.data, raw.size) == k * N.PN_STRIDE
    return X.cpu().numpy(), infos, P.state_from_device(raw_state(L)), N.state_from_device(raw, k)


def lambdas_run(L, A, At, s, B, lams, precond=P.PRECOND_NONE, X0=None, max_iter=0, diag=None, tol=None):
    """fs_pcgn_lambdas through capi.pcgn_lambdas: X (F, k), the infos, st[] by name, the per-column scalars by name"""
    from libfastsparse_amd import capi
    k = B.shape[1]
    Bd = to_device(B)
    X = nan_vector(s.ncol * k).view(s.ncol, k) if X0 is None else to_device(X0)
    dd = None if diag is None else to_device(diag)
    infos = capi.pcgn_lambdas(A, At, X, Bd, lams, s.tol if tol is None else tol, max_iter=max_iter, precond=precond,
                              warm_start=X0 is not None, diag=dd, stream=capi.current_stream())
    raw = np.full(N.MAX_RHS * N.PN_STRIDE, np.nan)
    assert L.fs_debug_last_pcgn_state(raw.ctypes.data, raw.size) == k * N.PN_STRIDE
    return X.cpu().numpy(), infos, P.state_from_device(raw_state(L)), N.state_from_device(raw, k)


def mscg_run(L, A, At, s, lams, max_iter=0, tol=None, ldx=None):
    """fs_mscg through capi.mscg: X (m, F), the infos, st[] by name, the per-shift array by name"""
    from libfastsparse_amd import capi
    m, F = len(lams), s.ncol
    ldx = F if ldx is None else ldx
    X = nan_vector(m * ldx).as_strided((m, F), (ldx, 1))
    infos = capi.mscg(A, At, X, to_device(s.b), lams, s.tol if tol is None else tol, max_iter, capi.current_stream())
    raw = np.full(S.MAX_SHIFTS * S.MS_STRIDE, np.nan)
    assert L.fs_debug_last_mscg_state(raw.ctypes.data, raw.size) == m * S.MS_STRIDE
    return X.cpu().numpy(), infos, S.state_from_device(raw_state(L)), S.shifts_from_device(raw, m)


def mscgn_state(L, k, m):
    """per column of the last fs_mscgn / fs_dist_mscgn solve: (st[] by name, the per-shift array by name)"""
    cols = []
    for j in range(k):
        st, raw = np.full(M.CG_STATE_DOUBLES, np.nan), np.full(S.MAX_SHIFTS * S.MS_STRIDE, np.nan)
        assert L.fs_debug_last_mscgn_state(j, st.ctypes.data, raw.ctypes.data, raw.size) == m * S.MS_STRIDE
        cols.append((S.state_from_device(st), S.shifts_from_device(raw, m)))
    return cols


def mscgn_run(L, A, At, s, B, lams, max_iter=0, tol=None):
    """fs_mscgn through capi.mscgn: X (m, F, k), infos[i][j], and per column (st[] by name, the per-shift array by name)"""
    from libfastsparse_amd import capi
    m, (F, k) = len(lams), B.shape
    X = nan_vector(m * F * k).view(m, F, k)
    infos = capi.mscgn(A, At, X, to_device(B), lams, s.tol if tol is None else tol, max_iter, capi.current_stream())
    return X.cpu().numpy(), infos, mscgn_state(L, k, m)


# ---- the models of fs_cg, once per case ------------------------------------------------------------------------------------
_CG_MODELS = {}


def cg_model(s, two, t="coo", bounds=None):
    key = (s.name, two, t, None if bounds is None else tuple(bounds))
    if key not in _CG_MODELS:
        t_csr = s.t_csr_coo() if t == "coo" else s.t_csr_sorted() if t == "sorted" else t
        _CG_MODELS[key] = s.model(two, t_csr=t_csr, bounds=bounds)
    return _CG_MODELS[key]


# ---- the assert helpers ----------------------------------------------------------------------------------------------------
def residual(s, x, lam=None):
    """||(A'A + lam I) x - b|| / ||b|| with the oracle's products (lam: the system's own unless given)"""
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), s.t_csr_coo())
    return float(np.linalg.norm(atm(am(x)) + (s.lam if lam is None else lam) * x - s.b) / np.linalg.norm(s.b))


def assert_cg_model(entry, s, two, x, it, st, model):
    bad = M.mismatch(x, model.x, it, model.iterations, st, model.state)
    assert bad is None, f"{entry} on {s.name} ({'cg2' if two else 'cg'}): {bad}"


def assert_exact(entry, mode, s, scale, two, x, it, st):
    what = f"{entry} [{mode}] on {s.name}"
    assert it == 0, (what, it)
    if not two:
        assert st["done"] == 1.0 and st["iter"] == 0.0 and st["alpha"] == 1.0 / scale, (what, st)
        assert M.same_bits(x, s.b / scale).all(), f"{what}: {M.mismatch(x, s.b / scale)}"
        return
    # cg2: Alpha = solve2sym(2^e R'R, R'R) with R'R diagonal (B's columns have disjoint supports): a0 = ((1 / (A0 A1)) A1) R'R0,
    # four roundings; R = B (1 / norm), X = (a0 R) norm: four more -- |X - B / 2^e| <= 8 u |B / 2^e| up to second order
    want = s.B / scale
    assert st["done"] == 1.0 and st["RtR[2]"] == 0.0, (what, st)
    err = np.abs(x - want)
    assert np.all(err <= 8 * 2.0 ** -53 * np.abs(want) * (1 + 1e-12)), (what, float(np.max(err / np.maximum(np.abs(want), 1e-300))))


def assert_info(what, info, model):
    st = model.state
    assert info.iterations == model.iterations and info.converged == int(st["done"]), (what, info.iterations, info.converged, st)
    assert M.same_bits(info.rnorm, np.sqrt(st["rr"]))[0] and M.same_bits(info.bnorm, np.sqrt(st["bb"]))[0], (what, info.rnorm, info.bnorm, st)


def assert_infos(what, infos, want):
    assert len(infos) == len(want), what
    for i, (g, w) in enumerate(zip(infos, want)):
        assert g.iterations == w.iterations and g.converged == w.converged, (what, i, g.iterations, g.converged, w)
        assert M.same_bits(g.rnorm, w.rnorm)[0] and M.same_bits(g.bnorm, w.bnorm)[0], (what, i, g.rnorm, g.bnorm, w)


def assert_column(what, x, info, cs, want_x, want_info, want_state=None):
    """column j of fs_pcgn / fs_pcgn_lambdas: x, its info and its scalars against fs_pcg's (the model's or the device's)"""
    ok = M.same_bits(x, want_x)
    assert ok.all(), (what, int((~ok).sum()), int(np.flatnonzero(~ok)[0]), x[~ok][:3], np.asarray(want_x)[~ok][:3])
    assert info.iterations == want_info.iterations and info.converged == want_info.converged, (what, info.iterations, info.converged, want_info)
    assert M.same_bits(info.rnorm, want_info.rnorm)[0] and M.same_bits(info.bnorm, want_info.bnorm)[0], (what, info.rnorm, info.bnorm, want_info)
    assert cs["count"] == want_info.iterations and cs["converged"] == want_info.converged, (what, cs)
    for key, name in (("rr", "rr"), ("bb", "bb"), ("stop", "stop"), ("rsq", "rz"), ("alpha", "alpha"), ("beta", "beta")):
        if want_state is not None and key in want_state:
            assert M.same_bits(cs[name], want_state[key])[0], (what, key, cs[name], want_state[key])


def assert_ladder_column(what, X, infos, col, want_X, want_infos, want_state, want_shifts):
    """column j of fs_mscgn: X (m, F), its m infos, (st, shifts) against fs_mscg's (the model's or the device's)"""
    st, shifts = col
    bad = M.mismatch(X, want_X, [i.iterations for i in infos], [i.iterations for i in want_infos], st, want_state)
    assert bad is None, f"{what}: {bad}"
    bad = S.shifts_mismatch(shifts, want_shifts)
    assert bad is None, f"{what}: {bad}"
    assert_infos(what, infos, want_infos)


def written(st):
    """the scalars of a device st[] of fs_mscg that such a solve is sure to have written: one that is done at the start writes no
    alpha, one without a second iteration no beta (those slots hold what the allocation held)"""
    never = set()
    if st["iter"] == 0.0:
        never.add("beta")
        if st["done"] == 1.0 and M.same_bits(st["rr"], st["bb"])[0]:
            never.add("alpha")
    return {key: v for key, v in st.items() if key not in never}


def same_solve(what, got, want):
    """two solves of fs_pcgn / fs_pcgn_lambdas (or their sharded forms): X, the infos and cs[], bit for bit"""
    (X, infos, _, cs), (Xw, infos_w, _, cs_w) = got, want
    assert M.same_bits(X, Xw).all(), (what, "X")
    for j, (a, b) in enumerate(zip(infos, infos_w)):
        assert (a.iterations, a.converged) == (b.iterations, b.converged), (what, j, a.iterations, b.iterations)
        assert M.same_bits(a.rnorm, b.rnorm)[0] and M.same_bits(a.bnorm, b.bnorm)[0], (what, j)
        for name in N.PN:
            assert M.same_bits(cs[j][name], cs_w[j][name])[0], (what, j, name, cs[j][name], cs_w[j][name])
