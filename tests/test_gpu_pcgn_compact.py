"""Option "pcgn_compact": fs_pcgn and fs_pcgn_lambdas move their live columns into narrower panels (include/fastsparse_hip.h, fs_pcgn,
"Narrowing"; the schedule is libfastsparse_amd/csrc/fs_pcgn_plan.h, modelled in tests/_pcgn_plan_model.py).  On the harness of
tests/_solvers.py.

1  strict_order, option 1 against option 0 in the same test: X, every fs_pcg_info, st[] and cs[] bit for bit, and
   capi.pcgn_segments() equal to the plan model fed with the solve's own counts; both forms of the kernels where k > 4.  The
   power-law ladder (k = 8, three widths or more) and its two-rung form (k = 2 down to width 1); k = 32 with a column frozen from
   the start; 17 -> 16 on F = 257 (a ragged last tile); a cap inside or right behind a repack; warm starts with a column that is
   converged at the start and keeps X0's bits; fs_pcgn with one lambda; a repack before iteration 0 on more than one grid stride.
2  default and reproducible modes on the two ladders with option 1: every column converged, true residual <= 2 tol, the count
   within one of the model's; a second solve repeats the bits and the segments.
3  option 1 where nothing finishes early: one segment, and the bits of option 0 in every mode.
4  statuses: every FS_ERR_ARG leaves X untouched with option 1; a released handle on which only k was prepared still solves, on a
   ladder without the rungs it cannot prepare; guard zones around X, B, diag and the lambdas; no device memory is kept."""
import ctypes as C

import numpy as np
import pytest

import _cg_model as M
import _gpu as G
import _lifecycle as LC
import _pcg_model as P
import _pcgn_lambdas_model as NL
import _pcgn_model as N
import _pcgn_plan_model as PM
import _solvers as SV
from _gpu import FS_ERR_ARG, FS_ERR_RELEASED, FS_OK

pytestmark = pytest.mark.gpu

NONE, JACOBI, DIAG = P.PRECOND_NONE, P.PRECOND_JACOBI, P.PRECOND_DIAG
CASE = {name: i for i, (name, _, _, _) in enumerate(SV.CASES)}


@pytest.fixture(scope="module")
def L():
    lib = G.gpu_lib()
    assert lib.fs_get_option(b"pcgn_compact") == 0, "the default of option pcgn_compact is 0"
    return lib


def rungs_below(k):
    return [w for w in PM.RUNGS if w < k]


def solve(L, A, At, s, B, lams, compact, precond=NONE, X0=None, max_iter=0, diag=None):
    """one solve under option pcgn_compact = `compact`: (X, infos, st, cs), the live mask of st[], the segments.  lams None: fs_pcgn"""
    from libfastsparse_amd import capi
    with G.options(pcgn_compact=compact):
        if lams is None:
            got = SV.pcgn_run(L, A, At, s, B, precond, X0, max_iter, diag)
        else:
            got = SV.lambdas_run(L, A, At, s, B, lams, precond, X0, max_iter, diag)
    return got, SV.raw_state(L)[N.ST_PCGN["live_mask"]], capi.pcgn_segments()


def assert_same_solve(what, one, zero):
    """option 1 against option 0: X, the infos, st[] and cs[] bit for bit"""
    (got, mask, _), (want, mask_w, segs_w) = one, zero
    SV.same_solve(what, got, want)
    for name in got[2]:
        assert M.same_bits(got[2][name], want[2][name])[0], (what, "st", name, got[2][name], want[2][name])
    assert mask == mask_w, (what, "live mask", mask, mask_w)
    k = got[0].shape[1]
    assert segs_w == [(0, k, PM.all_columns(k))], (what, "option 0 has one segment", segs_w)


def assert_plan(what, one, k, cap, usable=None):
    (_, infos, _, cs), _, segs = one
    want = PM.of_solve(k, rungs_below(k) if usable is None else usable, infos, cs, cap)
    print(what, "counts", [i.iterations for i in infos], "segments", segs)
    assert segs == want, (what, segs, want, [i.iterations for i in infos])
    return segs


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def _both(L, s, B, lams, kernel, precond=NONE, X0=None, max_iter=0, diag=None):
    with G.options(strict_order=1, pcgn_kernel=kernel):
        A, At = SV.handles(L, s)
        zero = solve(L, A, At, s, B, lams, 0, precond, X0, max_iter, diag)
        one = solve(L, A, At, s, B, lams, 1, precond, X0, max_iter, diag)
    return one, zero


@pytest.mark.parametrize("kernel", SV.KERNELS, ids=[f"pcgn_kernel{v}" for v in SV.KERNELS])
def test_strict_the_powerlaw_ladder(L, kernel):
    s, lams, B, model = SV.ladder("powerlaw_seed0")
    one, zero = _both(L, s, B, lams, kernel, JACOBI)
    assert_same_solve((s.name, kernel), one, zero)
    segs = assert_plan((s.name, kernel), one, 8, s.ncol)
    assert [i.iterations for i in one[0][1]] == [i.iterations for i in model.infos]
    assert len({w for _, w, _ in segs}) >= 3, segs
    assert [(a, w) for a, w, _ in segs] == [(0, 8), (12, 4), (18, 2)], segs           # checked by hand in tests/test_pcgn_plan.py


def test_strict_two_rungs_reach_width_one(L):
    s, lams, B, model = SV.ladder("powerlaw_seed0")
    one, zero = _both(L, s, np.ascontiguousarray(B[:, :2]), [lams[0], lams[7]], 0, JACOBI)
    assert_same_solve((s.name, "two rungs"), one, zero)
    segs = assert_plan((s.name, "two rungs"), one, 2, s.ncol)
    assert segs[-1][1] == 1 and segs[-1][2] == 0b01, segs
    assert [i.iterations for i in one[0][1]] == [model.infos[0].iterations, model.infos[7].iterations]


STRICT = [("fixture_100x50", 32, "diag"), ("binary_F257", 17, "jacobi"), ("binary_F65", 5, "jacobi-cap5"), ("valued", 8, "jacobi-warm"),
          ("valued", 8, "diag-warm-cap3")]
STRICT_RUNS = [(n, k, c, v) for n, k, c in STRICT for v in SV.KERNELS]


@pytest.mark.parametrize("name,k,case,kernel", STRICT_RUNS, ids=[f"{n}-k{k}-{c}-pcgn_kernel{v}" for n, k, c, v in STRICT_RUNS])
def test_strict_option_1_is_option_0(L, name, k, case, kernel):
    s = SV.ALL[name]
    what, precond, warm, max_iter = SV.CASES[CASE[case]]
    diag = SV.caller_diag(s) if precond == DIAG else None
    lams = NL.rungs(s, k)
    B = SV.columns(s, k)
    X0 = None
    done0 = (3, 4, 5, 6) if warm else ()                          # columns that start from a solution: converged at the start
    if warm:
        X0 = SV.x0_columns(s, B)
        with G.options(strict_order=1):
            A, At = SV.handles(L, s)
            tight = SV.lambdas_run(L, A, At, s, B, lams, precond, None, 0, diag, tol=s.tol * 1e-3)
        assert all(tight[1][j].converged == 1 for j in done0)
        X0[:, done0] = tight[0][:, done0]
    one, zero = _both(L, s, B, lams, kernel, precond, X0, max_iter, diag)
    assert_same_solve((name, k, what, kernel), one, zero)
    segs = assert_plan((name, k, what, kernel), one, k, max_iter or s.ncol)
    X, infos = one[0][0], one[0][1]
    assert infos[2].iterations == 0 and infos[2].converged == 1 and M.same_bits(X[:, 2], np.zeros(s.ncol)).all(), (name, k, what)
    for j in done0:
        assert infos[j].iterations == 0 and infos[j].converged == 1 and M.same_bits(X[:, j], X0[:, j]).all(), (name, k, what, j, infos[j].iterations)
    if name == "binary_F257":
        assert segs[0][:2] == (0, 16), segs                       # the zero column is frozen from the start: 17 -> 16 before iteration 0
    if max_iter:
        assert all(i.iterations <= max_iter for i in infos)
    assert len(segs) >= 2 or segs[0][1] < k, (name, k, what, "the case does not narrow", segs)


def test_strict_fs_pcgn_with_one_lambda(L):
    """fs_pcgn keeps its scalar-lambda kernels in every segment; columns scaled by powers of ten, so that their sums differ"""
    s = SV.ALL["valued"]
    B = SV.columns(s, 8) * (10.0 ** np.arange(-4, 4))[None, :]
    for kernel in SV.KERNELS:
        one, zero = _both(L, s, B, None, kernel, JACOBI)
        assert_same_solve((s.name, "fs_pcgn", kernel), one, zero)
        assert_plan((s.name, "fs_pcgn", kernel), one, 8, s.ncol)


def test_strict_a_repack_before_the_first_iteration_on_more_than_one_grid_stride(L):
    s = SV.ALL["binary_F262145"]
    assert s.ncol > M.RED_BLOCKS * M.RED_THREADS
    B = np.stack([s.b, np.zeros(s.ncol)], 1)
    one, zero = _both(L, s, B, [s.lam, s.lam * 30.0], 0, JACOBI, max_iter=3)
    assert_same_solve((s.name, "k 2"), one, zero)
    segs = assert_plan((s.name, "k 2"), one, 2, 3)
    assert segs == [(0, 1, 0b01)], segs
    infos = one[0][1]
    assert (infos[0].iterations, infos[0].converged, infos[1].iterations, infos[1].converged) == (3, 0, 0, 1)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("default", "reproducible"))
@pytest.mark.parametrize("name", ("scaled_seed0", "powerlaw_seed0"))
def test_the_ladders_with_option_1_within_the_bars(L, name, mode):
    s, lams, B, model = SV.ladder(name)
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), s.t_csr_coo())
    assert all(i.converged == 1 for i in model.infos)
    with G.mode_options(mode):
        A, At = SV.handles(L, s)
        runs = [solve(L, A, At, s, B, lams, 1, JACOBI) for _ in range(2)]
    (X, infos, _, _), _, segs = runs[0]
    nb = np.linalg.norm(s.b)
    for j, lam in enumerate(lams):
        info = infos[j]
        res = float(np.linalg.norm(atm(am(X[:, j])) + lam * X[:, j] - s.b) / nb)
        print(f"{name} [{mode}] rung {j} (lambda {lam:g}): {info.iterations} iterations (model {model.infos[j].iterations}), true residual "
              f"{res / s.tol:.2f} tol")
        what = (name, mode, j, lam, info.iterations, model.infos[j].iterations, res)
        assert info.converged == 1, what
        assert res <= 2 * s.tol, what
        assert abs(info.iterations - model.infos[j].iterations) <= 1, what
        assert info.rnorm <= s.tol * info.bnorm, what
    assert_plan((name, mode), runs[0], 8, s.ncol)
    assert len(segs) >= 2, segs
    # fixed-order products: a solve repeats its bits, and with them its counts and its segments
    assert M.same_bits(runs[1][0][0], X).all() and [i.iterations for i in runs[1][0][1]] == [i.iterations for i in infos], (name, mode)
    assert runs[1][2] == segs, (name, mode, runs[1][2], segs)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_nothing_finishes_early_one_segment_and_the_bits_of_option_0(L, mode):
    s = SV.ALL["valued"]
    for k in (4, 8):
        B = np.ascontiguousarray(np.repeat(s.b[:, None], k, 1))
        for lams in ([s.lam * 3.0] * k, None):
            with G.mode_options(mode):
                A, At = SV.handles(L, s)
                zero, again = [solve(L, A, At, s, B, lams, 0, JACOBI) for _ in range(2)]
                one = solve(L, A, At, s, B, lams, 1, JACOBI)
            if mode != "cg_fixed_order=0" or M.same_bits(again[0][0], zero[0][0]).all():   # where option 0 repeats its own bits
                assert_same_solve((mode, k, lams is None), one, zero)
            assert one[2] == [(0, k, PM.all_columns(k))], (mode, k, one[2])
            assert all(i.converged == 1 for i in one[0][1])


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_statuses(L):
    from libfastsparse_amd import capi
    s = SV.RECIPES["scaled_seed0"]
    A, At = SV.handles(L, s)
    st = capi.current_stream()
    k = 3
    B = G.to_device(SV.columns(s, k))
    X, d = G.nan_vector(s.ncol * N.MAX_RHS), G.to_device(SV.caller_diag(s))
    x_bits = X.cpu().numpy().view(np.int64).copy()
    good = NL.rungs(s, k)

    def call(A_=A.h, At_=At.h, x_=X.data_ptr(), b_=B.data_ptr(), k_=k, lams=good, prm="default", info=None, **kw):
        if prm == "default":
            f = dict(tol=1e-8, max_iter=0, precond=JACOBI, warm_start=0, diag=None)
            f.update(kw)
            prm = C.byref(capi.PcgParams(f["tol"], f["max_iter"], f["precond"], f["warm_start"], f["diag"]))
        if lams == "fs_pcgn":
            return L.fs_pcgn(A_, At_, x_, b_, k_, s.lam, prm, info, st)
        lam = None if lams is None else (C.c_double * N.MAX_RHS)(*(list(lams) + [1.0] * (N.MAX_RHS - len(lams))))
        return L.fs_pcgn_lambdas(A_, At_, x_, b_, k_, lam, prm, info, st)

    with G.options(pcgn_compact=1):
        bad = {"NULL A": call(A_=None), "NULL At": call(At_=None), "NULL X": call(x_=None), "NULL B": call(b_=None), "NULL prm": call(prm=None),
               "NULL lambda": call(lams=None), "At of A's shape": call(At_=A.h), "k 0": call(k_=0), "k -1": call(k_=-1), "k 33": call(k_=33),
               "lambda NaN": call(lams=good[:2] + [float("nan")]), "lambda inf": call(lams=good[:2] + [float("inf")]),
               "precond 3": call(precond=3), "precond -1": call(precond=-1), "DIAG without diag": call(precond=DIAG),
               "tol < 0": call(tol=-1e-8), "tol NaN": call(tol=float("nan")),
               "fs_pcgn NULL A": call(A_=None, lams="fs_pcgn"), "fs_pcgn k 33": call(k_=33, lams="fs_pcgn"),
               "fs_pcgn At of A's shape": call(At_=A.h, lams="fs_pcgn"), "fs_pcgn precond 3": call(precond=3, lams="fs_pcgn"),
               "fs_pcgn tol < 0": call(tol=-1e-8, lams="fs_pcgn")}
        assert all(rc == FS_ERR_ARG for rc in bad.values()), bad
        SV.refused_call_leaves(X, x_bits)
        infos = (capi.PcgInfo * k)()
        assert call(tol=0.0, max_iter=2, info=infos) == FS_OK          # tol = 0 is legal: the cap ends it
        assert [i.iterations for i in infos] == [2, 2, 0] and [i.converged for i in infos] == [0, 0, 1]
        assert capi.pcgn_segments() == [(0, 2, 0b011)]               # column 2 is zero: two live columns from the start
        assert call(precond=NONE, diag=d.data_ptr(), max_iter=1, lams="fs_pcgn") == FS_OK
    assert L.fs_get_option(b"pcgn_compact") == 0


def test_a_released_handle_solves_on_the_rungs_it_has(L):
    """fs_matrix_release_csr on a kept two-pass A' on which only k was prepared: the solve still answers FS_OK with option 1, on a
    ladder without the rungs whose one-time work now answers FS_ERR_RELEASED, silently.  Which rungs those are is the handle's
    business (a k-column copy that was never built, a plan that falls back to the row kernel): the test asks the handle the way the
    solve does -- fs_matrix_prepare on both sides, and the plan fs_spmm would run -- and feeds the answer to the plan model.
    k = 4 where the released handle still multiplies four columns, else k = 3."""
    from libfastsparse_amd import capi
    s = SV.RECIPES["scaled_seed0"]
    st = capi.current_stream()
    trp, tcc, tvv = s.t_csr_coo()
    r = NL.rungs(s, 8)
    kept = P.gram_diag(s.t_csr_coo(), s.lam)
    row_kernels = (1, 4)                                             # plans of fs_matrix_spmm_plan that read the plain CSR

    def pair():
        A, _ = SV.handles(L, s)
        At = capi.Matrix.from_csr(s.ncol, s.nrow, G.to_device(trp), G.to_device(tcc), G.to_device(tvv))
        assert At.kernel_name() == "two-pass"
        return A, At

    def usable_now(A, At, w):
        if w >= 2 and (L.fs_matrix_prepare(A.h, w, 0, st) != FS_OK or L.fs_matrix_prepare(At.h, w, 0, st) != FS_OK):
            assert L.fs_matrix_prepare(At.h, w, 0, st) == FS_ERR_RELEASED
            return False
        return w == 1 or L.fs_matrix_spmm_plan(At.h, w, 0) not in row_kernels

    with G.options(binning=2, bin_flags=64):                         # a kept two-pass copy: there is something to release for
        for k in (4, 3):
            lams = [r[6], r[4], r[0], r[0]][:k]                       # (one diagonal for all columns: the small rungs converge with it)
            B = np.ascontiguousarray(np.repeat(s.b[:, None], k, 1))
            A, At = pair()
            before = solve(L, A, At, s, B, lams, 0, DIAG, diag=kept)  # prepares k and nothing else
            assert At.release_csr() == 1
            if usable_now(A, At, k):
                break
        usable = [w for w in rungs_below(k) if usable_now(A, At, w)]
        print(f"released two-pass A': k = {k}, usable rungs {usable}")
        after = solve(L, A, At, s, B, lams, 1, DIAG, diag=kept)       # FS_OK: capi raises on anything else
        segs = assert_plan("after the release", after, k, s.ncol, usable=usable)
        assert {w for _, w, _ in segs} <= set(usable) | {k}, (segs, usable)
        assert all(i.converged == 1 for i in after[0][1])
        A2, At2 = pair()                                             # the same solve on handles that were never released
        full = solve(L, A2, At2, s, B, lams, 1, DIAG, diag=kept)
        segs_full = assert_plan("full ladder", full, k, s.ncol)
        assert len(segs_full) >= 2, segs_full
        # Jacobi needs the plain CSR of A' itself: refused before anything is written, with option 1 as without
        X = G.nan_vector(s.ncol * k)
        bits = X.cpu().numpy().view(np.int64).copy()
        jac = capi.PcgParams(s.tol, 0, JACOBI, 0, None)
        with G.options(pcgn_compact=1):
            assert L.fs_pcgn_lambdas(A.h, At.h, X.data_ptr(), G.to_device(B).data_ptr(), k, (C.c_double * k)(*lams), C.byref(jac), None,
                                     st) == FS_ERR_RELEASED
        SV.refused_call_leaves(X, bits, "the refused Jacobi solve wrote to X")


def test_guard_zones(L):
    """X, B and diag inside guard zones, 16-byte aligned and 8 bytes off, both forms of the kernels, option 1: guards untouched, the
    inputs unchanged, and the result 8 bytes off has the bits of the aligned one"""
    import torch
    from libfastsparse_amd import capi
    mem = LC.TorchMem()
    st = capi.current_stream()
    s = SV.ALL["binary_F257"]
    A, At = SV.handles(L, s)
    diag = SV.caller_diag(s)
    n = s.ncol * 5
    gx, gb, gd = (LC.Guarded(mem, "X of fs_pcgn_lambdas", n), LC.Guarded(mem, "B of fs_pcgn_lambdas", n),
                  LC.Guarded(mem, "diag of fs_pcgn_lambdas", s.ncol))
    narrowed = 0
    for kernel, k in [(v, k) for v in SV.KERNELS for k in (3, 5)]:
        B = SV.columns(s, k)
        X0 = SV.x0_columns(s, B)
        lams = NL.rungs(s, k)
        host = np.full(k + 16, np.nan)
        host.view(np.int64)[:] = LC.guard_bits(0x1A3B)
        host[8:8 + k] = lams
        host_bits = host.view(np.int64).copy()
        for what, precond, warm, max_iter in SV.CASES:
            aligned = None
            for off in (0, 1):
                mem.put(gb.place(s.ncol * k, off), B.reshape(-1))
                mem.put(gd.place(s.ncol, off ^ 1), diag)
                if warm:
                    mem.put(gx.place(s.ncol * k, off), X0.reshape(-1))
                else:
                    mem.fill_bits(gx.place(s.ncol * k, off), LC.PREFILLS["nan"])
                prm = capi.PcgParams(s.tol, max_iter, precond, int(warm), gd.view.data_ptr() if precond == DIAG else None)
                infos = (capi.PcgInfo * k)()
                with G.options(pcgn_kernel=kernel, pcgn_compact=1):
                    capi.check(L.fs_pcgn_lambdas(A.h, At.h, gx.view.data_ptr(), gb.view.data_ptr(), k,
                                                 C.cast(host.ctypes.data + 64, C.POINTER(C.c_double)), C.byref(prm), infos, st), "fs_pcgn_lambdas")
                torch.cuda.synchronize()
                segs = capi.pcgn_segments()
                narrowed += len(segs) > 1 or segs[0][1] < k
                where = (s.name, kernel, k, what, off)
                bad = mem.first_bad_guard([gx, gb, gd])
                assert bad is None, (where, bad.first_broken())
                assert mem.eq(gb.view, mem.const(B.reshape(-1))) and mem.eq(gd.view, mem.const(diag)), (where, "an input changed")
                assert np.array_equal(host.view(np.int64), host_bits), (where, "the lambdas or their neighbours changed")
                got = mem.get(gx.view)
                assert np.isfinite(got).all(), where
                if aligned is None:
                    aligned = (got.copy(), [i.iterations for i in infos], segs)
                else:
                    assert M.same_bits(got, aligned[0]).all() and [i.iterations for i in infos] == aligned[1], (where, "differs from off = 0")
                    assert segs == aligned[2], (where, segs, aligned[2])
    assert narrowed >= 8, narrowed


def test_no_device_memory_is_kept(L):
    import torch
    from libfastsparse_amd import capi
    s = SV.RECIPES["powerlaw_seed0"]
    A, At = SV.handles(L, s)
    st = capi.current_stream()
    k = 8
    lams = NL.rungs(s, k)
    B = G.to_device(np.repeat(s.b[:, None], k, 1))
    X, d = torch.empty_like(B), G.to_device(SV.caller_diag(s))

    def solves():
        for precond in (JACOBI, NONE, DIAG):
            infos = capi.pcgn_lambdas(A, At, X, B, lams, s.tol, precond=precond, diag=d, stream=st)
            assert all(i.converged == 1 for i in infos), precond
            assert len(capi.pcgn_segments()) >= 2, precond

    with G.options(pcgn_compact=1):
        solves()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(10):
            solves()
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
    print(f"free device memory: {free0} bytes after the first solves, {free1} after 30 solves more")
    assert free1 == free0, (free0, free1)
