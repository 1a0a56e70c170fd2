"""What the sharded solver suites share (tests/test_gpu_dist_{pcg,mscg,pcgn_lambdas,mscgn,pair}.py): sharded handles on virtual
ranks of one device, the runners of the sharded solvers, their model caches, and the frames that recur from suite to suite -- the
products counted, a handle without a transposed side, interleaved solves that give their memory back.
The single-device half is tests/_solvers.py, the device basics are tests/_gpu.py.

torch and libfastsparse_amd are imported inside the functions: the module itself imports on a machine without a GPU."""
import contextlib
import ctypes as C

import numpy as np

import _cg_model as M
import _dist_mscg_model as DS
import _dist_pair as DPair
import _dist_pcg_model as DP
import _mscg_model as S
import _pcg_model as P
import _pcgn_model as N
import _solvers as SV
from _gpu import options, put, to_numpy
from _solvers import GAP_BITS, split_rows_and_gaps, strided_rows

# ---- the systems -----------------------------------------------------------------------------------------------------------
RECIPES0 = {n: s for n, s in SV.RECIPES.items() if n.endswith("seed0")}
ALL = dict({n: SV.SYSTEMS[n] for n in SV.DIST_SET}, **RECIPES0)
# the systems of the sharded ladder suites
MSCG_RECIPES0 = {n: SV.RECIPES[n] for n in ("control_seed0", "powerlaw_seed0")}
MSCG_ALL = dict({n: SV.SYSTEMS[n] for n in SV.DIST_SET}, **MSCG_RECIPES0)
PAIR_SYSTEMS = {n: ALL[n] for n in DPair.NAMED + DPair.RECIPES0}
KS = (1, 2, 3, 4, 5, 8, 17, 32)


def panel(k):
    """the control recipe and k columns from _pcgn_model.recipe8's panel (a tiny and a huge column, a zero one, the top eigenvector:
    columns that freeze at different iterations), taken round and round with another scale each time"""
    s, B8, _ = N.recipe8("control")
    return s, np.ascontiguousarray(np.stack([B8[:, j % 8] * (1.0 + 0.25 * (j // 8)) for j in range(k)], 1))


# ---- the handles -----------------------------------------------------------------------------------------------------------
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
        return (x.reshape(-1, 2) if two else x), it.value, SV.cg_state(self.L, two)

    def close(self):
        self.L.fs_dist_matrix_destroy(self.M)
        self.L.fs_dist_destroy(self.D)


def dev_rows(nrow, ranks):
    """route `dev`: the rows of A per rank, an empty shard in the middle"""
    return [nrow] if ranks == 1 else [nrow // 2, 0, nrow - nrow // 2] + [0] * (ranks - 3)


def from_shards(L, D, nrow, ncol, csr, rows, space):
    """fs_dist_csr_create_from_shards on the CSR cut into `rows` rows per rank: local row_ptr from 0, global column ids; the arrays
    in host memory, or (FS_DEVICE) uploaded with torch"""
    import torch
    from libfastsparse_amd import capi
    rp, cc, vv = csr
    n = len(rows)
    cut = [0] + [int(v) for v in np.cumsum(rows)]
    assert cut[-1] == nrow
    keep, ptrs, nnzs = [], ([], [], []), []
    for r in range(n):
        lo, hi = int(rp[cut[r]]), int(rp[cut[r + 1]])
        nnzs.append(hi - lo)
        arrays = (np.ascontiguousarray(rp[cut[r]:cut[r + 1] + 1] - lo, np.int32), np.ascontiguousarray(cc[lo:hi], np.int32),
                  None if vv is None else np.ascontiguousarray(vv[lo:hi], np.float64))
        for a, out in zip(arrays, ptrs):
            if a is not None and space == capi.FS_DEVICE:
                a = torch.from_numpy(a).cuda()
            keep.append(a)
            out.append(capi._ptr(a))
    if space == capi.FS_DEVICE:
        torch.cuda.synchronize()
    vp = C.c_void_p * n
    h = L.fs_dist_csr_create_from_shards(D, nrow, ncol, (C.c_int * n)(*rows), (C.c_int64 * n)(*nnzs), vp(*ptrs[0]), vp(*ptrs[1]),
                                         None if vv is None else vp(*ptrs[2]), space)
    assert h, L.fs_last_error()
    return h


class PairDist(Dist):
    """Dist on a pair: .M = fs_dist_matrix_pair(.A, .At) on fs_dist_create(ranks).  Routes:
      coo   A fs_dist_csr_create from s.a_csr(); At fs_dist_coo_create(D, ncol, nrow, nnz, s.cols, s.rows, s.vals): the rows of A' in
            the caller's entry order, s.t_csr_coo(), cut by non-zeros
      cuts  the same A; At fs_dist_csr_create_from_shards (host arrays) from s.t_csr_coo() with the caller's cuts, _dist_pair.cut_rows
      dev   A fs_dist_csr_create_from_shards from arrays uploaded with torch, an empty shard in the middle; At as in `coo`
    s: a _cg_model.System, or anything with its nrow, ncol, rows, cols, vals, a_csr() and t_csr_coo()"""

    def __init__(self, L, s, ranks, route):
        from libfastsparse_amd import capi
        assert route in DPair.ROUTES, route
        self.L, self.s, self.ranks, self.route = L, s, ranks, route
        self.csr, self.t_want = s.a_csr(), s.t_csr_coo()
        self.A = self.At = self.M = None
        self.D = L.fs_dist_create(ranks, (C.c_int * ranks)(*([0] * ranks)))
        assert self.D, L.fs_last_error()
        try:
            rp, cc, vv = self.csr
            vals = None if s.vals is None else s.vals.ctypes.data
            if route == "dev":
                self.A = from_shards(L, self.D, s.nrow, s.ncol, self.csr, dev_rows(s.nrow, ranks), capi.FS_DEVICE)
            else:
                self.A = L.fs_dist_csr_create(self.D, s.nrow, s.ncol, len(cc), rp.ctypes.data, cc.ctypes.data, None if vv is None else vv.ctypes.data)
            assert self.A, L.fs_last_error()
            if route == "cuts":
                self.At = from_shards(L, self.D, s.ncol, s.nrow, self.t_want, DPair.cut_rows(s.ncol, ranks), capi.FS_HOST)
            else:
                self.At = L.fs_dist_coo_create(self.D, s.ncol, s.nrow, s.rows.size, s.cols.ctypes.data, s.rows.ctypes.data, vals)
            assert self.At, L.fs_last_error()
            self.M = capi.dist_matrix_pair(self.A, self.At)
        except BaseException:
            self.close()
            raise

    def bounds_of(self, h):
        b = (C.c_int * (self.ranks + 1))()
        assert self.L.fs_dist_matrix_bounds(h, b) == 0
        return list(b)

    def bounds_t(self):
        """the pair's cuts of A' are At's own cuts of its rows: the caller's, or (fs_dist_coo_create) the cut by non-zeros"""
        b = super().bounds_t()
        want = DPair.cut_bounds(self.s.ncol, self.ranks) if self.route == "cuts" else DPair.nnz_bounds(self.t_want[0], self.ranks)
        assert b == self.bounds_of(self.At) == want, (self.route, b, self.bounds_of(self.At), want)
        return b

    def t_csr(self):
        """the pair's transposed shards, downloaded: the caller's A' array for array -- the caller's order, not a sorted one"""
        t = super().t_csr()
        assert DPair.same_arrays(t, self.t_want), (getattr(self.s, "name", "?"), self.route, self.ranks, "the shards of A' are not the caller's arrays")
        return t

    def close(self):
        for h in (self.M, self.A, self.At):
            if h:
                self.L.fs_dist_matrix_destroy(h)
        self.M = self.A = self.At = None
        self.L.fs_dist_destroy(self.D)


def sorted_t(dist, s):
    t_csr, want = dist.t_csr(), s.t_csr_sorted()
    assert all(np.array_equal(a, b) for a, b in zip(t_csr[:2], want[:2])), (s.name, "A' rows are not in ascending A-row order")
    return t_csr


@contextlib.contextmanager
def handle_without_transpose(L, dist, s):
    """a second handle of A on dist's ranks that has no transposed side"""
    rp, cc, vv = s.a_csr()
    M_not = L.fs_dist_csr_create(dist.D, s.nrow, s.ncol, len(cc), rp.ctypes.data, cc.ctypes.data, vv.ctypes.data)
    assert M_not
    try:
        yield M_not
    finally:
        L.fs_dist_matrix_destroy(M_not)


# ---- the entry points ------------------------------------------------------------------------------------------------------
def dpcg(L, dist, s, precond=P.PRECOND_NONE, x0=None, max_iter=0, diag=None, tol=None, b=None, hbm=False):
    """fs_dist_pcg through capi.dist_pcg: x, fs_pcg_info, rank 0's final st[] by name"""
    from libfastsparse_amd import capi
    x = put(np.full(s.ncol, np.nan) if x0 is None else x0, hbm)
    bd = put(s.b if b is None else b, hbm)
    dd = None if diag is None else put(diag, hbm)
    info = capi.dist_pcg(dist.M, x, bd, s.lam, s.tol if tol is None else tol, max_iter=max_iter, precond=precond, warm_start=x0 is not None,
                         diag=dd)
    return to_numpy(x), info, P.state_from_device(SV.raw_state(L))


def dpcgn(L, dist, s, B, precond=P.PRECOND_NONE, X0=None, max_iter=0, diag=None, tol=None, hbm=False):
    """fs_dist_pcgn through capi.dist_pcgn: X (F, k), the infos, st[] by name, rank 0's per-column scalars by name"""
    from libfastsparse_amd import capi
    k = B.shape[1]
    X = put(np.full(B.shape, np.nan) if X0 is None else X0, hbm)
    infos = capi.dist_pcgn(dist.M, X, put(B, hbm), s.lam, s.tol if tol is None else tol, max_iter=max_iter, precond=precond,
                           warm_start=X0 is not None, diag=None if diag is None else put(diag, hbm))
    raw = np.full(N.MAX_RHS * N.PN_STRIDE, np.nan)
    assert L.fs_debug_last_pcgn_state(raw.ctypes.data, raw.size) == k * N.PN_STRIDE
    return to_numpy(X), infos, P.state_from_device(SV.raw_state(L)), N.state_from_device(raw, k)


def dnl(L, dist, s, B, lams, precond=P.PRECOND_NONE, X0=None, max_iter=0, diag=None, tol=None, hbm=False):
    """fs_dist_pcgn_lambdas through capi.dist_pcgn_lambdas: X (F, k), the infos, st[] by name, rank 0's per-column scalars by name"""
    from libfastsparse_amd import capi
    k = B.shape[1]
    X = put(np.full(B.shape, np.nan) if X0 is None else X0, hbm)
    infos = capi.dist_pcgn_lambdas(dist.M, X, put(B, hbm), lams, s.tol if tol is None else tol, max_iter=max_iter, precond=precond,
                                   warm_start=X0 is not None, diag=None if diag is None else put(diag, hbm))
    raw = np.full(N.MAX_RHS * N.PN_STRIDE, np.nan)
    assert L.fs_debug_last_pcgn_state(raw.ctypes.data, raw.size) == k * N.PN_STRIDE
    return to_numpy(X), infos, P.state_from_device(SV.raw_state(L)), N.state_from_device(raw, k)


def dmscg(L, dist, s, lams, max_iter=0, tol=None, b=None, hbm=False, ldx=None):
    """fs_dist_mscg through capi.dist_mscg: X (m, F), the infos, rank 0's st[] by name and per-shift array by name.  X lies in one
    buffer of (m - 1) ldx + F doubles, host memory or HBM; the gaps between the x_i must keep their bits"""
    from libfastsparse_amd import capi
    m, F = len(lams), s.ncol
    ldx = F if ldx is None else ldx
    buf, X = strided_rows(m, F, ldx, hbm, GAP_BITS)
    infos = capi.dist_mscg(dist.M, X, put(s.b if b is None else b, hbm), lams, s.tol if tol is None else tol, max_iter)
    raw = np.full(S.MAX_SHIFTS * S.MS_STRIDE, np.nan)
    assert L.fs_debug_last_mscg_state(raw.ctypes.data, raw.size) == m * S.MS_STRIDE
    rows, gaps = split_rows_and_gaps(buf, m, F, ldx)
    assert (gaps.view(np.int64) == GAP_BITS).all(), "a gap between the x_i was written"
    return rows, infos, S.state_from_device(SV.raw_state(L)), S.shifts_from_device(raw, m)


def dmscgn(L, dist, s, B, lams, max_iter=0, tol=None, hbm=False, ldx=None):
    """fs_dist_mscgn through capi.dist_mscgn: X (m, F, k), infos[i][j], per column rank 0's (st[] by name, per-shift array by name),
    and the solve's st[] by fs_pcg's names.  X lies in one buffer of (m - 1) ldx + F k doubles, host memory or HBM; the gaps between
    the panels must keep their bits"""
    from libfastsparse_amd import capi
    m, (F, k) = len(lams), B.shape
    ne = F * k
    ldx = ne if ldx is None else ldx
    buf, X = strided_rows(m, (F, k), ldx, hbm, GAP_BITS)
    infos = capi.dist_mscgn(dist.M, X, put(B, hbm), lams, s.tol if tol is None else tol, max_iter)
    cols = SV.mscgn_state(L, k, m)
    rows, gaps = split_rows_and_gaps(buf, m, ne, ldx)
    assert (gaps.view(np.int64) == GAP_BITS).all(), "a gap between the panels was written"
    return rows.reshape(m, F, k), infos, cols, P.state_from_device(SV.raw_state(L))


# ---- the cases and models of the sharded solvers, once per case ------------------------------------------------------------
def case_args(s, case, t_csr):
    what, precond, warm, max_iter = SV.CASES[case]
    diag = None
    if precond == P.PRECOND_DIAG:
        d = P.gram_diag(t_csr, s.lam)
        diag = np.abs(d) * (1.0 + 0.5 * np.cos(np.arange(s.ncol) * 1.7)) + 0.125
    return what, precond, (SV.x0(s) if warm else None), max_iter, diag


_DPCG_MODELS = {}
_DMSCG_MODELS = {}
DNL_CACHE = {}                                                       # of _dist_pcgn_lambdas_model.run


def dpcg_model(s, case, t_csr, bounds=None):
    """the (slice) model of a case on the A' the shards hold; the sorted A' is the same for every rank count and either build (the
    entries of A' are part of the key: a pair handle holds the caller's order, tests/test_gpu_dist_pair.py)"""
    key = (s.name, case, None if bounds is None else tuple(bounds), t_csr[1].tobytes(), None if t_csr[2] is None else t_csr[2].tobytes())
    if key not in _DPCG_MODELS:
        _, precond, x0, max_iter, diag = case_args(s, case, t_csr)
        _DPCG_MODELS[key] = DP.run(s, precond, max_iter=max_iter, x0=x0, t_csr=t_csr, diag=diag, bounds=bounds)
    return _DPCG_MODELS[key]


def dmscg_model(s, ladder, cap, t_csr, bounds=None, lams=None, tol=None):
    """the (slice) model of a solve on the A' the shards hold, once per case"""
    key = (s.name, ladder, cap, tol, None if bounds is None else tuple(bounds), t_csr[1].tobytes(), None if t_csr[2] is None else t_csr[2].tobytes())
    if key not in _DMSCG_MODELS:
        _DMSCG_MODELS[key] = DS.run(s, SV.lams_of(s, ladder) if lams is None else lams, max_iter=cap, tol=tol, t_csr=t_csr, bounds=bounds)
    return _DMSCG_MODELS[key]


# ---- the assert helpers ----------------------------------------------------------------------------------------------------
def assert_dmscg_model(what, got, model):
    X, infos, st, shifts = got
    bad = M.mismatch(X, model.X, [i.iterations for i in infos], [i.iterations for i in model.infos], st, model.state)
    assert bad is None, f"{what}: {bad}"
    bad = S.shifts_mismatch(shifts, model.shifts)
    assert bad is None, f"{what}: {bad}"
    SV.assert_infos(what, infos, model.infos)


def assert_dnl_model(what, got, model, columns=None):
    X, infos, st, cs = got
    for j in (range(X.shape[1]) if columns is None else columns):
        SV.assert_column((what, j, "model"), X[:, j], infos[j], cs[j], model.X[:, j], model.infos[j], model.columns[j].state)
    if columns is None:
        assert st["iter"] == max(i.iterations for i in infos) and st["done"] == float(all(c["live"] == 0.0 for c in cs)), (what, st)


def assert_default_mode_bars(L, dist, s):
    """the bars of a column-scaled recipe in the default mode, both schemes, on any handle with a transposed side (a built one in
    test_gpu_dist_pcg.py, a pair in test_gpu_dist_pair.py)"""
    name = s.name
    model = P.run(s, P.PRECOND_JACOBI)
    assert model.state["done"] == 1.0
    for scheme in (0, 1):
        with options(dist_cg_scheme=scheme):
            runs = [dpcg(L, dist, s, P.PRECOND_JACOBI) for _ in range(2)]
            plain = dpcg(L, dist, s)
        x, info, _ = runs[0]
        res = SV.residual(s, x)
        print(f"{name} scheme {scheme}: jacobi {info.iterations} iterations (model {model.iterations}), true residual {res:.3g} "
              f"= {res / s.tol:.2f} tol; plain {plain[1].iterations} iterations, converged {plain[1].converged}")
        what = (name, scheme, info.iterations, model.iterations, res)
        assert info.converged == 1, what
        assert res <= 2 * s.tol, what
        assert abs(info.iterations - model.iterations) <= 1, what
        assert info.rnorm <= s.tol * info.bnorm, what
        assert runs[1][1].iterations == info.iterations and M.same_bits(runs[1][0], x).all(), what
        assert plain[1].converged == 0 and plain[1].iterations == s.ncol, (what, plain[1].iterations)


# ---- the products counted --------------------------------------------------------------------------------------------------
def loops(cap, iterations, at_start=False):
    """iterations the host enqueues: the device sets `done` in loop iteration j and reports iterations == j; the host sees the flags of
    iteration j synchronously behind iteration j + 1, so j + 2 iterations were enqueued -- or the cap; none for a solve done at its start"""
    return 0 if at_start else min(cap, iterations + 2)


def counted(L, f):
    """f(), and the sharded products it issued (fs_debug_dist_products)"""
    before = L.fs_debug_dist_products()
    out = f()
    return L.fs_debug_dist_products() - before, out


# ---- interleaved solves ----------------------------------------------------------------------------------------------------
def with_scheme(scheme, f):
    def run():
        with options(dist_cg_scheme=scheme):
            return f()
    return run


def interleaved_then_memory_back(L, s, ranks, kinds, seed, allowance, unchecked=None):
    """kinds(dist): solves on one handle, each returning its X.  A first handle: each once, then in a seeded random order between the
    others, with the bits of its first run.  A second handle (whatever the process keeps for good exists by now): each once -- or
    unchecked(dist) in their place -- and after its destroy free device memory is back where it was before it existed, within
    `allowance` bytes"""
    import torch

    def cycle(check):
        dist = Dist(L, s, ranks, False)
        try:
            if unchecked is not None and not check:
                unchecked(dist)
                return
            fs = kinds(dist)
            first = [f() for f in fs]
            if check:
                order = np.random.default_rng(seed).permutation(len(fs) * 2) % len(fs)
                for i in order:
                    assert M.same_bits(fs[i](), first[i]).all(), f"solve kind {i} changed its bits between other solves"
        finally:
            dist.close()

    cycle(True)                                                      # (warm-up: whatever the process keeps for good exists now)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    cycle(False)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print(f"free device memory: {free0} bytes before the handle, {free1} after its destroy; allowance {allowance}")
    assert free0 - free1 <= allowance, (free0, free1, allowance)


class CutPair(Dist):
    """fs_dist_matrix_pair(A, At): A from s.a_csr(), At from s.t_csr_coo() -- the caller's entry order -- cut at the caller's `bounds`"""

    def __init__(self, L, s, bounds):
        from libfastsparse_amd import capi
        ranks = len(bounds) - 1
        self.L, self.s, self.ranks = L, s, ranks
        self.csr = s.a_csr()
        self.A = self.At = self.M = None
        self.D = L.fs_dist_create(ranks, (C.c_int * ranks)(*([0] * ranks)))
        assert self.D, L.fs_last_error()
        try:
            rp, cc, vv = self.csr
            self.A = L.fs_dist_csr_create(self.D, s.nrow, s.ncol, len(cc), rp.ctypes.data, cc.ctypes.data, None if vv is None else vv.ctypes.data)
            assert self.A, L.fs_last_error()
            self.At = from_shards(L, self.D, s.ncol, s.nrow, s.t_csr_coo(), [b - a for a, b in zip(bounds, bounds[1:])], capi.FS_HOST)
            self.M = capi.dist_matrix_pair(self.A, self.At)
        except BaseException:
            self.close()
            raise

    def close(self):
        for h in (self.M, self.A, self.At):
            if h:
                self.L.fs_dist_matrix_destroy(h)
        self.M = self.A = self.At = None
        self.L.fs_dist_destroy(self.D)


def assert_dmscgn_model(what, got, model, columns=None):
    """dmscgn's outcome against _dist_mscgn_model.run's: every column's X, infos, st[] and per-shift array, then the solve's st[]"""
    X, infos, cols, st = got
    k = X.shape[2]
    assert X.shape == model.X.shape and len(infos) == X.shape[0] and all(len(r) == k for r in infos), what
    for j in (range(k) if columns is None else columns):
        c = model.columns[j]
        SV.assert_ladder_column(f"{what}, column {j}", X[:, :, j], [row[j] for row in infos], cols[j], c.X, c.infos, c.state, c.shifts)
    if columns is None:
        assert st["iter"] == max(c.state["iter"] for c in model.columns), (what, st)
        assert st["done"] == float(all(c.state["done"] == 1.0 for c in model.columns)), (what, st)


# ---- sharded solves on dirty work space (tests/test_gpu_dist_dirty_work.py) -------------------------------------------------
SOLVERS = ("cg", "cg2", "pcg", "pcgn", "pcgn_lambdas", "mscg", "mscgn")
READS_SCHEME = ("cg", "pcg", "pcgn_lambdas", "mscg", "mscgn")        # fs_dist_cg2 and fs_dist_pcgn are replicated whatever it says
K_COLUMN = ("cg2", "pcgn", "pcgn_lambdas", "mscgn")
LADDER = ("mscg", "mscgn")
PCG_FAMILY = ("pcg", "pcgn", "pcgn_lambdas")
MN_SCALARS = 9344                                                    # the header's "9344 doubles of scalars" of fs_dist_mscgn


def work_space_per_rank(solver, F, nrow, bounds, k=1, m=1, nslots=0, scheme=0):
    """the doubles of every device buffer a sharded solve keeps on its handle, all ranks' (include/fastsparse_hip.h, "Work space per
    rank", with the sizes ensure_cg_work / ensure_pn_work / ensure_ladder_work / ensure_k of fs_dist.hip ask for): what poison_heap
    fills before a solve that makes, or re-makes, them"""
    n = len(bounds) - 1
    rows = [b - a for a, b in zip(bounds, bounds[1:])]
    slices = scheme == 1 and n > 1 and solver in READS_SCHEME
    kk = 2 if solver == "cg2" else k if solver in K_COLUMN else 1
    out = [F, nrow]                                                  # fs_dist_x / _y / _z
    if solver in ("cg", "pcg", "mscg"):                              # CgWork: sol, r, b, p, q, dinv with room for a window; the sums
        out += [F + max(rows) + 1, M.CG_PART_DOUBLES, 3 * DP.SEND_DOUBLES, DP.SEND_DOUBLES * n + 1, M.CG_STATE_DOUBLES]
    if kk > 1 or solver in K_COLUMN:                                 # KWork: the whole P, T, Q of the k-column products; fs_dist_cg2's own
        out += [F * kk, nrow * kk, M.CG_PART_DOUBLES, 4, M.CG_STATE_DOUBLES]
    if solver in ("pcgn", "pcgn_lambdas", "mscgn"):                  # PnWork
        for r in (rows if slices else [F]):
            out += [max(r, 1) * k, max(r, 1)]
        out += [2 * M.RED_BLOCKS * k, N.MAX_RHS * N.PN_STRIDE, M.CG_STATE_DOUBLES]
        if slices:
            out += [2 * 2 * N.MAX_RHS, n * 2 * N.MAX_RHS]
    if solver in LADDER:                                             # LadderWork: m x_i, nslots P_i of ld doubles, the scalars
        ld = ((max(rows) if slices else F) * (k if solver == "mscgn" else 1) + 1) & ~1
        out += [ld * m, ld * max(nslots, 1), S.MAX_SHIFTS * S.MS_STRIDE if solver == "mscg" else MN_SCALARS]
    return sorted({v for v in out if v > 0})


class DirtyFrame:
    """One sharded handle and the caller's vectors of its solves, every vector inside guard zones (LC.Guarded) in host memory or in
    HBM.  solve(): one call of a sharded solver by its C entry point; after it the guards of X, B and diag are intact, B and diag
    are unchanged, the gaps between the panels of X keep their bits, and a refused call leaves all of X with its prefill.
    check(): the outcome against the solver's model bit for bit -- X, the infos, rank 0's state from the debug hooks."""

    def __init__(self, L, dist, s, t_csr, bounds, kmax=8):
        import _lifecycle as LC
        self.LC, self.L, self.dist, self.s, self.t_csr, self.bounds = LC, L, dist, s, t_csr, [int(b) for b in bounds]
        F = s.ncol
        self.F = F
        self.mems = {False: LC.NumpyMem(), True: LC.TorchMem()}
        self.vec = {(hbm, role): LC.Guarded(mem, f"{role} of a sharded solve in {'HBM' if hbm else 'host memory'}", cap)
                    for hbm, mem in self.mems.items() for role, cap in (("X", S.MAX_SHIFTS * (F * kmax + 3)), ("B", F * kmax), ("diag", F))}
        self.products = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr)
        self.tkey = (s.name, t_csr[1].tobytes(), None if t_csr[2] is None else t_csr[2].tobytes())
        self.solves = 0

    def solve(self, solver, B, lam=None, lams=None, tol=None, cap=0, precond=P.PRECOND_NONE, X0=None, diag=None, hbm=False, pad=0, raw=None):
        """(status, X as the solver's model shapes it or None, the infos or [count])"""
        from libfastsparse_amd import capi
        import torch
        LC, L, s, F = self.LC, self.L, self.s, self.F
        hbm = hbm and solver not in ("cg", "cg2")                    # (fs_dist_cg / _cg2 take host vectors)
        B = np.ascontiguousarray(B, np.float64)
        k = B.shape[1] if B.ndim == 2 else 1
        m = len(lams) if solver in LADDER else 1
        ne = F * k
        ldx = ne + pad if solver in LADDER else ne
        nx = (m - 1) * ldx + ne
        gx, gb, gd = (self.vec[(hbm, role)] for role in ("X", "B", "diag"))
        mem = self.mems[hbm]
        before = np.full(nx, LC.PREFILLS["nan"], np.int64).view(np.float64)
        if X0 is not None:
            before = np.ascontiguousarray(X0, np.float64).reshape(-1).copy()
        off8 = self.solves & 1
        self.solves += 1
        mem.put(gx.place(nx, off8), before)
        mem.put(gb.place(B.size, off8 if k > 1 else (self.solves >> 1) & 1), B.reshape(-1))
        ins = [(gb, B.reshape(-1), "B")]
        if diag is not None:
            mem.put(gd.place(F, (self.solves >> 2) & 1), diag)
            ins.append((gd, np.ascontiguousarray(diag, np.float64), "diag"))
        if hbm:
            torch.cuda.synchronize()
        tol = s.tol if tol is None else tol
        lam = s.lam if lam is None else lam
        a = dict(M=self.dist.M, X=mem.ptr(gx.view), B=mem.ptr(gb.view), k=k, m=m, ldx=ldx, tol=tol, cap=cap, precond=precond,
                 lams=None if lams is None else [float(v) for v in lams])
        a.update(raw or {})
        prm = capi.PcgParams(float(a["tol"]), int(a["cap"]), int(a["precond"]), int(X0 is not None), None if diag is None else mem.ptr(gd.view))
        infos = (capi.PcgInfo * max(m * k, 1))()
        arr = None if a["lams"] is None else (C.c_double * max(len(a["lams"]), 1))(*a["lams"])
        it = C.c_int(-1)
        if solver in ("cg", "cg2"):
            rc = getattr(L, "fs_dist_" + solver)(a["M"], a["X"], a["B"], lam, a["tol"], C.byref(it))
        elif solver == "pcg":
            rc = L.fs_dist_pcg(a["M"], a["X"], a["B"], lam, C.byref(prm), infos)
        elif solver == "pcgn":
            rc = L.fs_dist_pcgn(a["M"], a["X"], a["B"], a["k"], lam, C.byref(prm), infos)
        elif solver == "pcgn_lambdas":
            rc = L.fs_dist_pcgn_lambdas(a["M"], a["X"], a["B"], a["k"], arr, C.byref(prm), infos)
        elif solver == "mscg":
            rc = L.fs_dist_mscg(a["M"], a["X"], a["ldx"], a["B"], a["m"], arr, a["tol"], a["cap"], infos)
        else:
            rc = L.fs_dist_mscgn(a["M"], a["X"], a["ldx"], a["B"], a["k"], a["m"], arr, a["tol"], a["cap"], infos)
        what = f"fs_dist_{solver}"
        for g in (gx, gb, gd):
            assert g.guards_ok(), (what, g.first_broken())
        for g, want, name in ins:
            assert g.mem.eq(g.view, g.mem.const(want)), (what, f"the caller's {name} was modified")
        got = mem.get(gx.view)
        if rc != 0:
            assert np.array_equal(got.view(np.int64), before.view(np.int64)), (what, rc, "a refused call wrote to X")
            return rc, None, None
        if solver in LADDER:
            gaps = np.ones(nx, bool)
            for i in range(m):
                gaps[i * ldx:i * ldx + ne] = False
            assert np.array_equal(got.view(np.int64)[gaps], before.view(np.int64)[gaps]), (what, "a gap between the panels of X was written")
            X = np.stack([got[i * ldx:i * ldx + ne] for i in range(m)])
            X = X.reshape(m, F, k) if solver == "mscgn" else X
            out = [list(infos[i * k:(i + 1) * k]) for i in range(m)] if solver == "mscgn" else list(infos)[:m]
        elif solver in ("cg", "cg2"):
            X, out = (got.reshape(F, 2) if solver == "cg2" else got), [it.value]
        else:
            X, out = (got.reshape(F, k) if solver != "pcg" else got), list(infos)[:k]
        return rc, X, out

    def column(self, kind, b, lam, lams, tol, cap, dinv, x0, bounds):
        """one column's model (_dist_pcg_model.pcg, _dist_mscg_model.mscg), kept by its arguments"""
        key = (self.tkey, kind, b.tobytes(), float(lam), None if lams is None else tuple(float(v) for v in lams), float(tol), cap,
               None if dinv is None else dinv.tobytes(), None if x0 is None else x0.tobytes(), None if bounds is None else tuple(bounds))
        if key not in _DIRTY_MODELS:
            am, atm, _, _ = self.products
            _DIRTY_MODELS[key] = (DP.pcg(self.F, am, atm, b, lam, tol, cap, dinv, x0, bounds) if kind == "pcg" else
                                  DS.mscg(self.F, am, atm, b, lams, tol, cap, bounds))
        return _DIRTY_MODELS[key]

    def check(self, what, solver, scheme, X, infos, B, lam=None, lams=None, tol=None, cap=0, precond=P.PRECOND_NONE, X0=None, diag=None):
        """the solve just made against its model, bit for bit: X, the infos, rank 0's state from the debug hooks"""
        import _mscgn_model as SN
        import _pcgn_lambdas_model as NL
        L, s, F = self.L, self.s, self.F
        tol = s.tol if tol is None else tol
        lam = s.lam if lam is None else lam
        B = np.ascontiguousarray(B, np.float64)
        k = B.shape[1] if B.ndim == 2 else 1
        bounds = self.bounds if scheme == 1 and self.dist.ranks > 1 and solver in READS_SCHEME else None
        am, atm, am2, atm2 = self.products
        if solver == "cg":
            key = (self.tkey, "cg", B.tobytes(), float(lam), float(tol), None if bounds is None else tuple(bounds))
            if key not in _DIRTY_MODELS:
                _DIRTY_MODELS[key] = M.cg(F, am, atm, B, lam, tol, "device", bounds)
            model = _DIRTY_MODELS[key]
            bad = M.mismatch(X, model.x, infos[0], model.iterations, SV.cg_state(L, False), model.state)
            assert bad is None, f"{what}: {bad}"
        elif solver == "cg2":
            key = (self.tkey, "cg2", B.tobytes(), float(lam), float(tol))
            if key not in _DIRTY_MODELS:
                _DIRTY_MODELS[key] = M.cg2(F, am2, atm2, B, lam, tol)
            model = _DIRTY_MODELS[key]
            bad = M.mismatch(X, model.x, infos[0], model.iterations, SV.cg_state(L, True), model.state)
            assert bad is None, f"{what}: {bad}"
        elif solver in PCG_FAMILY:
            Bc = B.reshape(F, k)
            X0c = None if X0 is None else np.ascontiguousarray(X0, np.float64).reshape(F, k)
            ls = [lam] * k if solver != "pcgn_lambdas" else list(lams)
            cols = [self.column("pcg", np.ascontiguousarray(Bc[:, j]), ls[j], None, tol, cap, NL.dinv_of_column(self.t_csr, ls[j], precond, diag),
                                None if X0c is None else np.ascontiguousarray(X0c[:, j]), bounds) for j in range(k)]
            st = P.state_from_device(SV.raw_state(L))
            if solver == "pcg":
                bad = M.mismatch(X, cols[0].x, infos[0].iterations, cols[0].iterations, st, cols[0].state)
                assert bad is None, f"{what}: {bad}"
                SV.assert_info(what, infos[0], cols[0])
            else:
                raw = np.full(N.MAX_RHS * N.PN_STRIDE, np.nan)
                assert L.fs_debug_last_pcgn_state(raw.ctypes.data, raw.size) == k * N.PN_STRIDE
                model = N.ResultN(np.stack([c.x for c in cols], 1), [N.info_of(c) for c in cols], cols)
                assert_dnl_model(what, (X, infos, st, N.state_from_device(raw, k)), model)
        elif solver == "mscg":
            model = self.column("mscg", B.reshape(F), 0.0, lams, tol, cap, None, None, bounds)
            raw = np.full(S.MAX_SHIFTS * S.MS_STRIDE, np.nan)
            assert L.fs_debug_last_mscg_state(raw.ctypes.data, raw.size) == len(lams) * S.MS_STRIDE
            assert_dmscg_model(what, (X, infos, S.state_from_device(SV.raw_state(L)), S.shifts_from_device(raw, len(lams))), model)
        else:
            Bc = B.reshape(F, k)
            cols = [self.column("mscg", np.ascontiguousarray(Bc[:, j]), 0.0, lams, tol, cap, None, None, bounds) for j in range(k)]
            assert_dmscgn_model(what, (X, infos, SV.mscgn_state(L, k, len(lams)), P.state_from_device(SV.raw_state(L))), SN._gather(cols, len(lams)))

    def resident_products_exact(self, what):
        """fs_dist_x / _y / _z are the solvers' work vectors: upload an integer x again, then fs_dist_spmv_resident and
        fs_dist_spmv_t_resident are exact on every rank"""
        L, s, dist = self.L, self.s, self.dist
        am, atm, _, _ = self.products
        x = (np.arange(s.ncol) * 7 % 23 - 11).astype(np.float64)
        y = am(x)
        z = atm(y)
        for r in range(dist.ranks):
            assert L.fs_copy_to_device(L.fs_dist_x(dist.M, r), x.ctypes.data, 8 * s.ncol) == 0
        assert L.fs_dist_spmv_resident(dist.M) == 0, L.fs_last_error()
        assert L.fs_dist_spmv_t_resident(dist.M) == 0, L.fs_last_error()
        for r in range(dist.ranks):
            gy, gz = np.full(s.nrow, np.nan), np.full(s.ncol, np.nan)
            assert L.fs_copy_to_host(gy.ctypes.data, L.fs_dist_y(dist.M, r), 8 * s.nrow) == 0
            assert L.fs_copy_to_host(gz.ctypes.data, L.fs_dist_z(dist.M, r), 8 * s.ncol) == 0
            assert np.array_equal(gy.view(np.int64), y.view(np.int64)) and np.array_equal(gz.view(np.int64), z.view(np.int64)), (what, r)


_DIRTY_MODELS = {}
