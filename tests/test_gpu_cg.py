"""Every CG entry point against the CPU model of its device arithmetic (tests/_cg_model.py).

(a) Under strict_order every product returns the oracle's storage-order bits, so a solve's x, its iteration count and its final
    scalars (st[], read back by fs_debug_last_cg_state) are a deterministic function the model restates: they must agree bit for
    bit -- fs_cg / fs_cg2 on handles, bsbm_cg / bsbm_cg2 through the drop-in on host structs, fs_dist_cg in both schemes and
    fs_dist_cg2 on one and three virtual ranks.
(b) On systems whose every dot is exact in any order (A'A = m I, m + lam = 2^e, dyadic b) the answer is exact in every mode:
    x = b / 2^e at iteration 0, and the iteration enqueued after convergence leaves it so.
(c) In the default modes, the bars: the residual, the distance to the model's x, the iteration count; fixed-order solves repeat
    their bits."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _cg_model as M

pytestmark = pytest.mark.gpu

FS_ERR_ARG = -2
ROW_PLAN = 1                                             # fs_matrix_spmm_plan code of the row kernel (storage-order sums)
SYSTEMS = M.systems()
MODES = ("default", "cg_fixed_order=0", "reproducible", "strict_order")
DIST_SET = ("fixture_100x50", "binary_F65", "binary_F262145", "ill_conditioned", "cap_tol0", "three_eigenvalues", "zero_rhs",
            "cg2_equal_columns", "lambda0_empty_column", "valued")


@pytest.fixture(scope="module")
def L():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from libfastsparse_amd import capi
    lib = capi.lib()
    lib.fs_debug_last_cg_state.argtypes = [C.c_void_p]
    lib.fs_debug_last_spmm_plan.argtypes = []
    return lib


@contextlib.contextmanager
def options(**kw):
    """set library options, restore the values they had on the way out (the getter pattern of test_gpu_exact.py)"""
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


def _state(L, two):
    L.fs_debug_last_cg_state.argtypes = [C.c_void_p]
    st = np.full(M.CG_STATE_DOUBLES, np.nan)
    assert L.fs_debug_last_cg_state(st.ctypes.data) == M.CG_STATE_DOUBLES
    return M.state_from_device(st, two)


def _assert_model(entry, s, two, x, it, st, model):
    bad = M.mismatch(x, model.x, it, model.iterations, st, model.state)
    assert bad is None, f"{entry} on {s.name} ({'cg2' if two else 'cg'}): {bad}"


def _cases(names=None, valued=True):
    out = []
    for n, s in SYSTEMS.items():
        if (names is None or n in names) and (valued or s.vals is None):
            out += [(n, False)] + ([(n, True)] if s.two else [])
    return out


def _ids(cases):
    return [f"{n}-{'cg2' if t else 'cg'}" for n, t in cases]


# ---- the entry points --------------------------------------------------------------------------------------------------
def fs_cg_run(L, s, two, t_sorted=False, b=None):
    """fs_cg / fs_cg2 on handles: from COO like HipDeviceBackend.cg (A' in the caller's entry order), or (t_sorted) from the CSR
    of A and the A' of fs_dist_matrix_build_transpose, as fs_dist_cg holds them.  Returns x, the count, the final st[]."""
    import torch
    from libfastsparse_amd import capi
    vals = None if s.vals is None else _d(s.vals)
    if t_sorted:
        (arp, acc, avv), (trp, tcc, tvv) = s.a_csr(), s.t_csr_sorted()
        A = capi.Matrix.from_csr(s.nrow, s.ncol, _d(arp), _d(acc), None if avv is None else _d(avv))
        At = capi.Matrix.from_csr(s.ncol, s.nrow, _d(trp), _d(tcc), None if tvv is None else _d(tvv))
    else:
        A = capi.Matrix.from_coo(s.nrow, s.ncol, _d(s.rows), _d(s.cols), vals)
        At = capi.Matrix.from_coo(s.ncol, s.nrow, _d(s.cols), _d(s.rows), vals)
    if L.fs_get_option(b"strict_order") == 1:
        assert A.kernel_name() == "stream" and At.kernel_name() == "stream", (A.kernel_name(), At.kernel_name())
    rhs = (s.B if two else s.b) if b is None else b
    bd = _d(rhs.reshape(-1))
    x = torch.full((rhs.size,), float("nan"), dtype=torch.float64, device="cuda")
    it = C.c_int(-1)
    L.fs_debug_last_spmm_plan()
    f = L.fs_cg2 if two else L.fs_cg
    capi.check(f(A.h, At.h, x.data_ptr(), bd.data_ptr(), s.lam, s.tol, C.byref(it), capi.current_stream()), "fs_cg")
    if two and L.fs_get_option(b"strict_order") == 1:
        assert L.fs_debug_last_spmm_plan() == ROW_PLAN
    out = x.cpu().numpy()
    return (out.reshape(-1, 2) if two else out), it.value, _state(L, two)


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
    state = _state(L, two)
    L.fs_invalidate(Bl)
    L.fs_invalidate(Blt)
    return (x.reshape(-1, 2) if two else x), it.value, state, held


class Dist:
    """fs_dist_create(ranks) and a matrix from the CSR of A, A' from the host arrays or built on the device"""

    def __init__(self, L, s, ranks, device_t):
        self.L, self.s, self.ranks = L, s, ranks
        self.csr = s.a_csr()
        rp, cc, vv = self.csr
        self.D = L.fs_dist_create(ranks, (C.c_int * ranks)(*([0] * ranks)))
        assert self.D, L.fs_last_error()
        self.M = L.fs_dist_csr_create(self.D, s.nrow, s.ncol, len(cc), rp.ctypes.data, cc.ctypes.data, None if vv is None else vv.ctypes.data)
        assert self.M, L.fs_last_error()
        rc = (L.fs_dist_matrix_build_transpose_device(self.M) if device_t else
              L.fs_dist_matrix_build_transpose(self.M, rp.ctypes.data, cc.ctypes.data, None if vv is None else vv.ctypes.data))
        assert rc == 0, L.fs_last_error()

    def bounds_t(self):
        b = (C.c_int * (self.ranks + 1))()
        assert self.L.fs_dist_matrix_bounds_t(self.M, b) == 0
        return list(b)

    def t_csr(self):
        """the rows of A' the shards hold (fs_dist_matrix_shard + fs_matrix_download), laid end to end"""
        from libfastsparse_amd import capi
        L, bounds = self.L, self.bounds_t()
        rps, ccs, vvs = [np.zeros(1, np.int64)], [], []
        for r in range(self.ranks):
            if bounds[r + 1] == bounds[r]:
                continue
            h = L.fs_dist_matrix_shard(self.M, r, 1)
            n, nnz = L.fs_matrix_nrow(h), L.fs_matrix_nnz(h)
            assert n == bounds[r + 1] - bounds[r], (r, n, bounds)
            rp, cc, vv = np.empty(n + 1, np.int32), np.empty(nnz, np.int32), np.full(nnz, np.nan)
            capi.check(L.fs_matrix_download(h, 0, rp.ctypes.data, cc.ctypes.data, vv.ctypes.data), "fs_matrix_download")
            rps.append(rp[1:].astype(np.int64) + rps[-1][-1])
            ccs.append(cc)
            vvs.append(vv)
        cat = lambda a, dt: np.concatenate(a).astype(dt) if a else np.zeros(0, dt)
        return cat(rps, np.int32), cat(ccs, np.int32), None if self.s.vals is None else cat(vvs, np.float64)

    def cg(self, two, b=None):
        s = self.s
        rhs = np.ascontiguousarray((s.B if two else s.b) if b is None else b, dtype=np.float64).reshape(-1)
        x = np.full(rhs.size, np.nan)
        it = C.c_int(-1)
        f = self.L.fs_dist_cg2 if two else self.L.fs_dist_cg
        assert f(self.M, x.ctypes.data, rhs.ctypes.data, s.lam, s.tol, C.byref(it)) == 0, self.L.fs_last_error()
        return (x.reshape(-1, 2) if two else x), it.value, _state(self.L, two)

    def close(self):
        self.L.fs_dist_matrix_destroy(self.M)
        self.L.fs_dist_destroy(self.D)


_MODELS = {}


def _model(s, two, t="coo", bounds=None):
    key = (s.name, two, t, None if bounds is None else tuple(bounds))
    if key not in _MODELS:
        t_csr = s.t_csr_coo() if t == "coo" else s.t_csr_sorted() if t == "sorted" else t
        _MODELS[key] = s.model(two, t_csr=t_csr, bounds=bounds)
    return _MODELS[key]


# ---- (a) strict_order: bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,two", _cases(), ids=_ids(_cases()))
def test_fs_cg_strict_is_the_model(L, name, two):
    s = SYSTEMS[name]
    with options(strict_order=1):
        x, it, st = fs_cg_run(L, s, two)
    _assert_model("fs_cg2" if two else "fs_cg", s, two, x, it, st, _model(s, two))


@pytest.mark.parametrize("name,two", _cases(valued=False), ids=_ids(_cases(valued=False)))
def test_dropin_bsbm_cg_strict_is_the_model(L, name, two):
    s = SYSTEMS[name]
    with options(strict_order=1):
        x, it, st, (a_csr, t_csr) = dropin_run(L, s, two)
    am, atm, am2, atm2 = M.csr_products(s.nrow, s.ncol, a_csr, t_csr)
    model = M.cg2(s.ncol, am2, atm2, s.B, s.lam, s.tol) if two else M.cg(s.ncol, am, atm, s.b, s.lam, s.tol)
    _assert_model("bsbm_cg2" if two else "bsbm_cg", s, two, x, it, st, model)


@pytest.mark.parametrize("device_t", [False, True], ids=["host-transpose", "device-transpose"])
@pytest.mark.parametrize("ranks", [1, 3])
def test_fs_dist_cg_replicate_strict_is_the_model_and_fs_cg(L, ranks, device_t):
    """scheme 0 ("replicate"): identical kernels on identical vectors -- the model's bits and fs_cg's on the same CSRs"""
    for name in DIST_SET:
        s = SYSTEMS[name]
        dist = Dist(L, s, ranks, device_t)
        try:
            t_csr = dist.t_csr()
            want_t = s.t_csr_sorted()
            assert all(np.array_equal(a, b) for a, b in zip(t_csr[:2], want_t[:2])), (name, "A' rows are not in ascending A-row order")
            with options(strict_order=1, dist_cg_scheme=0):
                for two in ((False, True) if s.two else (False,)):
                    x, it, st = dist.cg(two)
                    model = _model(s, two, "sorted")
                    entry = f"fs_dist_cg{'2' if two else ''} scheme 0, {ranks} ranks, {'device' if device_t else 'host'} A'"
                    _assert_model(entry, s, two, x, it, st, model)
                    if not two and not device_t:
                        xs, its, sts = fs_cg_run(L, s, False, t_sorted=True)
                        bad = M.mismatch(x, xs, it, its, st, sts)
                        assert bad is None, f"fs_dist_cg scheme 0 vs fs_cg on {name}: {bad}"
        finally:
            dist.close()


def test_fs_dist_cg_gather_strict_is_the_slice_model(L):
    """scheme 1 ("gather") on 3 ranks: every rank reduces its slice (the row cuts of A'), the rank values are added by stage 2"""
    for name in DIST_SET:
        s = SYSTEMS[name]
        for device_t in (False, True):
            dist = Dist(L, s, 3, device_t)
            try:
                bounds = dist.bounds_t()
                assert bounds[0] == 0 and bounds[-1] == s.ncol
                with options(strict_order=1, dist_cg_scheme=1):
                    x, it, st = dist.cg(False)
                _assert_model(f"fs_dist_cg scheme 1, 3 ranks, bounds {bounds}", s, False, x, it, st, _model(s, False, "sorted", bounds))
            finally:
                dist.close()


# ---- (b) exact answers in every mode ----------------------------------------------------------------------------------
EXACT = [(M.exact_system(), 4.0), (M.exact_system(m=7, lam=9.0, F=700, seed=17), 16.0), (M.exact_system(lam=0.5, nrow=0), 0.5)]


def _assert_exact(entry, mode, s, scale, two, x, it, st):
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


@pytest.mark.parametrize("mode", MODES)
def test_exact_systems_single_device(L, mode):
    for s, scale in EXACT:
        for two in (False, True):
            with _mode(mode):
                x, it, st = fs_cg_run(L, s, two)
                _assert_exact("fs_cg", mode, s, scale, two, x, it, st)
                x, it, st, _ = dropin_run(L, s, two)
                _assert_exact("bsbm_cg", mode, s, scale, two, x, it, st)


@pytest.mark.parametrize("mode", MODES)
def test_exact_systems_three_ranks(L, mode):
    for s, scale in EXACT[:2]:
        dist = Dist(L, s, 3, False)
        try:
            for scheme in (0, 1):
                with _mode(mode), options(dist_cg_scheme=scheme):
                    x, it, st = dist.cg(False)
                    _assert_exact(f"fs_dist_cg scheme {scheme}", mode, s, scale, False, x, it, st)
            with _mode(mode):
                x, it, st = dist.cg(True)
                _assert_exact("fs_dist_cg2", mode, s, scale, True, x, it, st)
        finally:
            dist.close()


# ---- (c) default modes: the bars --------------------------------------------------------------------------------------
def _residual(s, x, two):
    """||(A'A + lam I) x - b|| / ||b|| per column, with the oracle's products"""
    am, atm, am2, atm2 = M.csr_products(s.nrow, s.ncol, s.a_csr(), s.t_csr_coo())
    if two:
        r = atm2(am2(x)) + s.lam * x - s.B
        return np.linalg.norm(r, axis=0) / np.linalg.norm(s.B, axis=0)
    return np.array([np.linalg.norm(atm(am(x)) + s.lam * x - s.b) / np.linalg.norm(s.b)])


DEFAULT_CASES = [(n, t) for n, t in _cases() if not SYSTEMS[n].nan and not (t and n in ("binary_F1", "lambda0_empty_column"))]


@pytest.mark.parametrize("name,two", DEFAULT_CASES, ids=_ids(DEFAULT_CASES))
def test_default_modes_within_the_bars_of_the_model(L, name, two):
    s = SYSTEMS[name]
    model = _model(s, two)
    res_m = _residual(s, model.x, two)
    bnorm = np.linalg.norm(s.B if two else s.b, axis=0) if two else np.array([np.linalg.norm(s.b)])
    for mode in ("default", "cg_fixed_order=0"):
        with _mode(mode):
            runs = [fs_cg_run(L, s, two) for _ in range(2)]
        x, it, _ = runs[0]
        what = (name, two, mode, it, model.iterations)
        res = _residual(s, x, two)
        if s.converges and not (two and name == "three_eigenvalues"):   # (two columns on three unknowns: the cap ends it)
            assert np.all(res <= 2 * s.tol), (what, res)
        if s.lam > 0:                                           # ||(A'A + lam I)^-1|| <= 1 / lam: holds for any two x
            err = np.linalg.norm((x - model.x).reshape(s.ncol, -1), axis=0)
            assert np.all(err <= (res + res_m) * bnorm / s.lam * 1.01 + 1e-300), (what, err, res, res_m)
        if s.well:
            assert abs(it - model.iterations) <= 1, what
        else:
            assert it <= s.ncol, what
        if mode == "default":                                   # fixed-order products: a solve repeats its bits
            assert runs[1][1] == it and M.same_bits(runs[1][0], x).all(), what


# ---- statuses ----------------------------------------------------------------------------------------------------------------
def test_statuses(L):
    """fs_cg / fs_cg2 refuse a NULL argument and an At of A's own shape with FS_ERR_ARG and a message, before anything is written
    to x; out_iter = NULL is legal"""
    import torch
    from libfastsparse_amd import capi
    s = SYSTEMS["fixture_100x50"]
    A = capi.Matrix.from_coo(s.nrow, s.ncol, _d(s.rows), _d(s.cols), None)
    At = capi.Matrix.from_coo(s.ncol, s.nrow, _d(s.cols), _d(s.rows), None)
    st = capi.current_stream()
    for f, rhs in ((L.fs_cg, s.b), (L.fs_cg2, s.B)):
        b = _d(rhs.reshape(-1))
        x = torch.full((rhs.size,), float("nan"), dtype=torch.float64, device="cuda")
        x_bits = x.cpu().numpy().view(np.int64).copy()
        good = dict(A=A.h, At=At.h, x=x.data_ptr(), b=b.data_ptr())
        for what, kw in (("NULL A", dict(A=None)), ("NULL At", dict(At=None)), ("NULL x", dict(x=None)), ("NULL b", dict(b=None)),
                         ("At is A", dict(At=A.h))):
            a = dict(good, **kw)
            rc = f(a["A"], a["At"], a["x"], a["b"], s.lam, s.tol, None, st)
            assert rc == FS_ERR_ARG, (f.__name__, what, rc)
            assert L.fs_last_error().startswith(f.__name__.encode() + b":"), (f.__name__, what, L.fs_last_error())   # its own message
        assert np.array_equal(x.cpu().numpy().view(np.int64), x_bits), f"{f.__name__}: a refused call wrote to x"
        assert f(A.h, At.h, x.data_ptr(), b.data_ptr(), s.lam, s.tol, None, st) == 0, L.fs_last_error()   # out_iter NULL is legal


# ---- the drop-in on three virtual ranks -----------------------------------------------------------------------------------
def test_dropin_cg_across_three_ranks_in_a_child_process(L):
    """FASTSPARSE_NGPU=3 FASTSPARSE_DEVICES=0,0,0: bsbm_cg / bsbm_cg2 on the row-sharded path -- strict_order bits against the
    model, exact answers in every mode (tests/_dropin_ngpu.py, mode `cg`)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dropin_ngpu.py")
    env = dict(os.environ, FASTSPARSE_NGPU="3", FASTSPARSE_DEVICES="0,0,0")
    p = subprocess.run([sys.executable, child, "cg"], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), p.stdout[-3000:] + p.stderr[-3000:]
