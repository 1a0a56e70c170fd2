"""Random operation walks on long-lived handles, with every vector inside guard zones (helper; no test in here).

A walk keeps two or three matrix handles alive and steps them in random interleaving through every legal call of
include/fastsparse_hip.h: products (one vector, k columns, A'A, in parts, host vectors), prepare / release_prepared,
release_csr / restore_csr / download, option flips, stream changes, handles destroyed and created mid-walk.  The data are the
exactly summable sets of tests/_exact.py, so ONE bar -- equality of bits -- serves every mode and every order of additions.

Solver pairs: next to these handles a walk keeps two pairs (A, At) of SEPARATE handles, as fs_cg takes them (At made from the
transposed arrays), which live through the same operations and, besides, through fs_gram_diag, fs_cg, fs_cg2, fs_pcg, fs_mscg,
fs_pcgn, fs_pcgn_lambdas and fs_mscgn (the k-column solves in whatever form option "pcgn_kernel" has been flipped to, fs_pcgn and fs_pcgn_lambdas narrowing
or not as option "pcgn_compact" says: their segments are those of tests/_pcgn_plan_model.py on the widths the Model says are usable).  One pair holds a system of _cg_model.ExactFamily (binary, or its twin with values +-2), on which every solve is exact in
whatever mode the flips have left; the other the general system binary_F257, for solves under strict_order that are compared with
the models bit for bit (x, counts, info and the state of the fs_debug_last_*_state hooks).  Products on the pairs use
integer-valued vectors.  After every solver operation: guards, inputs unchanged, the expected bits -- or, on an error, x still its
prefill: "raised before anything is written" --, the options and fs_matrix_spmv_kernel as before, fs_matrix_device_bytes as the
header says, the next product on either handle exact.  Half of the solves run right after poison_heap, which fills freed device
memory of the sizes the solve will ask for with a tagged NaN: a work vector read before it is written shows as that tag in x.

Guarded vectors: every vector handed to the library (x, u, X, U, y, z, Y, Z, tmp, the arrays of a borrowed matrix, the host
vectors of fs_spmv_host) lies inside a larger allocation of its own, with at least GUARD doubles of a quiet NaN on both sides
whose payload names the vector.  After EVERY operation: the guards of all vectors are untouched, the inputs are unchanged, the
outputs have the exact bits (int64 views, compared where the vectors live).  A guard value that reaches a sum shows up as a NaN
in an output and its payload says whose guard it was.
Out of scope: a stray LOAD whose value is discarded cannot be seen by guards, and is not hunted with unmapped pages.

A model of the handle (Model) predicts for every operation "exact" or one status of the header (FS_ERR_RELEASED,
FS_ERR_NO_TRANSPOSE, FS_ERR_ARG); the walk asserts the status, and that the next product on the handle is exact again.

The same walk code runs on the real library (HipBackend, GPU tests) and on a numpy stand-in (tests/test_lifecycle_model.py),
which is how the harness is shown to have teeth without a GPU.

Replay: a WalkFailure carries data set, copy, seed, the failing step and the last 20 log lines; run_walk(..., upto=N) replays
the first N steps of the same seed.  Nothing is retried: the first failing check ends the walk."""
import collections
import contextlib
import re
import zlib

import numpy as np

import _cg_model as M
import _exact as E
import _mscg_model as S
import _pcg_model as P
import _pcgn_model as N
import _pcgn_plan_model as PM

GUARD = 4096                        # doubles on either side of a vector: 32 KiB, wider than one 1024-thread store of doubles
FS_OK, FS_ERR_ARG, FS_ERR_NO_TRANSPOSE, FS_ERR_RELEASED = 0, -2, -4, -5
STATUS_NAMES = {0: "FS_OK", -1: "FS_ERR_HIP", -2: "FS_ERR_ARG", -3: "FS_ERR_NO_DEVICE", -4: "FS_ERR_NO_TRANSPOSE", -5: "FS_ERR_RELEASED"}
KS = (2, 3, 4, 5, 8, 16, 17)
NC = 18                             # right-hand sides per data set: a product takes one column or a run of k of them
QNAN = 0x7FF8 << 48
GUARD_MARK = (0x6A << 40) | 0x5A    # guard = QNAN | GUARD_MARK | tag << 8
PREFILLS = {"nan": QNAN | 0x0F0F00000001, "-0.0": -(1 << 63)}
ROW_PLAN, KCOL_PLAN, MFMA_PLAN, LDSX_COLUMNS_PLAN = 1, 2, 4, 5

FLIPS = {"reproducible": (0, 1), "strict_order": (0, 1), "cg_fixed_order": (1, 0), "spmv_kernel": (0, 1, 2, 3, "own"),
         "spmm_kernel": (0, 1, 2, 3), "spmm_wide": (0, -1, 1), "ata_kernel": (0, 2), "tiled_flags": (0, 4),
         "pcgn_kernel": (0, 1, 2), "pcgn_compact": (0, 1)}          # first value: default

# forced copies beyond the PATHS table of test_gpu_exact.py: the builder's own choice
AUTO = "auto"

OPS = {"spmv": 10, "spmv_t": 10, "spmm": 12, "spmm_t": 12, "ata": 6, "spmv_part": 12, "spmm_part": 5, "spmv_host": 3, "spmv_t_host": 3,
       "dev_then_host": 3, "prepare": 6, "release_prepared": 4, "prepare_roundtrip": 2, "release_csr": 5, "restore_csr": 5, "download": 2,
       "flip": 10, "stream": 4, "churn": 2, "build_transpose": 3, "bad_arg": 2,
       # on the handles of a solver pair only (elsewhere their weight is 0)
       "gram_diag": 5, "cg": 6, "cg2": 5, "pcg": 8, "mscg": 5, "pcgn": 8, "pcgn_lambdas": 7, "mscgn": 5, "solve_strict": 8,
       "solve_bad_arg": 4}
SOLVER_OPS = ("gram_diag", "cg", "cg2", "pcg", "mscg", "pcgn", "pcgn_lambdas", "mscgn", "solve_strict", "solve_bad_arg")
EXACT_ONLY = ("cg", "cg2", "pcg", "mscg", "pcgn", "pcgn_lambdas", "mscgn")      # solves that need the exact family
PCGN_KS = (1, 2, 3, 4, 5, 8, 16, 17, 32)
MSCGN_KS = (1, 2, 3, 5, 8)
LADDERS = ("mscg", "mscgn")                            # X is m vectors / panels ldx doubles apart
K_COLUMNS = ("pcgn", "pcgn_lambdas", "mscgn")          # B is a row-major F x k panel
NARROWING = ("pcgn", "pcgn_lambdas")                   # the solvers that read option "pcgn_compact"
MSCGN_SCALARS = 9344                                   # fs_mscgn's scalars (the header's figure), in one block with its 2048 k partials
POISON_TAG = 0x7E57AB1E                                # the tag of poison_heap's NaN


class WalkFailure(AssertionError):
    def __init__(self, msg, step, kind):
        super().__init__(msg)
        self.step, self.kind = step, kind


def guard_bits(tag):
    return QNAN | GUARD_MARK | (tag << 8)


def guard_tag(bits):
    """the tag of a guard value found in an output (sign and quiet bit aside), or None"""
    b = int(bits) & ((1 << 48) - 1)
    return (b >> 8) & 0xFFFFFFFF if (b & ~(0xFFFFFFFF << 8)) == GUARD_MARK else None


# ---- where vectors live --------------------------------------------------------------------------------------------------
class NumpyMem:
    """host memory (the host vectors of fs_spmv_host; everything of the numpy stand-in)"""
    def empty(self, n):
        return np.empty(n, np.float64)

    def fill_bits(self, v, bits):
        v.view(np.int64)[...] = bits

    def put(self, v, a):
        v[...] = a

    def const(self, a):
        return np.ascontiguousarray(a)

    def eq(self, v, c):
        if v.dtype != np.float64:
            return bool(np.array_equal(v, c))
        return bool(np.array_equal(v.view(np.int64), c.view(np.int64)))

    def guards_ok(self, store, lo, hi, bits):
        s = store.view(np.int64)
        return bool((s[:lo] == bits).all() and (s[hi:] == bits).all())

    def first_bad_guard(self, gs):
        return next((g for g in gs if not g.guards_ok()), None)

    def all_bits(self, v, bits):
        return bool((v.view(np.int64) == bits).all())

    def get(self, v):
        return np.array(v, copy=True)

    def ptr(self, v):
        return v.ctypes.data

    def i32(self, v):
        return v.view(np.int32)


class TorchMem:
    """HBM, through torch; every check runs on torch's current stream, the stream the walk launches on"""
    def __init__(self):
        import torch
        self.t = torch

    def empty(self, n):
        return self.t.empty(n, dtype=self.t.float64, device="cuda")

    def fill_bits(self, v, bits):
        v.view(self.t.int64).fill_(bits)

    def put(self, v, a):
        v.copy_(self.t.from_numpy(np.ascontiguousarray(a)).view(v.dtype))

    def const(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a)).cuda()

    def eq(self, v, c):
        t = self.t
        if v.dtype != t.float64:
            return bool(t.equal(v, c))
        return bool(t.equal(v.view(t.int64), c.view(t.int64)))

    def guards_ok(self, store, lo, hi, bits):
        s = store.view(self.t.int64)
        return bool(((s[:lo] == bits).all() & (s[hi:] == bits).all()).item())

    def first_bad_guard(self, gs):
        """one wait for all of them: outside its vector an allocation holds nothing but its guard value (no vector holds one)"""
        gs = [g for g in gs if g.lo is not None]
        if not gs:
            return None
        t = self.t
        other = t.stack([(g.store.view(t.int64) != g.bits).sum() for g in gs]).tolist()
        for g, n in zip(gs, other):
            if n != g.hi - g.lo and not g.guards_ok():
                return g
        return None

    def all_bits(self, v, bits):
        return bool((v.view(self.t.int64) == bits).all().item())

    def get(self, v):
        return v.cpu().numpy()

    def ptr(self, v):
        return v.data_ptr()

    def i32(self, v):
        return v.view(self.t.int32)


TAGS = {POISON_TAG: "poison (solver work space read before it was written)"}     # tag -> name, for a guard value found in a sum


class Guarded:
    """`cap` doubles in the middle of their own allocation, guard zones of >= GUARD doubles of a tagged quiet NaN around them"""
    _next = [1]

    def __init__(self, mem, name, cap):
        self.mem, self.name, self.cap = mem, name, cap
        self.tag = Guarded._next[0]
        Guarded._next[0] += 1
        TAGS[self.tag] = name
        self.bits = guard_bits(self.tag)
        self.store = mem.empty(cap + 2 * GUARD + 2)
        self.base_odd = (mem.ptr(self.store) >> 3) & 1
        self.lo = self.hi = None
        self.view = None

    def place(self, n, off8=0):
        """guards over the whole allocation, then a vector of n doubles that starts 16-byte aligned (off8 = 0) or 8 bytes off"""
        assert 0 <= n <= self.cap, (self.name, n, self.cap)
        self.mem.fill_bits(self.store, self.bits)
        self.lo = GUARD + ((self.base_odd ^ off8) & 1)
        self.hi = self.lo + n
        self.view = self.store[self.lo:self.hi]
        assert n == 0 or self.mem.ptr(self.view) % 16 == 8 * off8
        return self.view

    def guards_ok(self):
        return self.lo is None or self.mem.guards_ok(self.store, self.lo, self.hi, self.bits)

    def first_broken(self):
        s = self.mem.get(self.store).view(np.int64)
        bad = np.flatnonzero(s != self.bits)
        bad = bad[(bad < self.lo) | (bad >= self.hi)]
        i = int(bad[0])
        where = f"{self.lo - i} double(s) before it" if i < self.lo else f"{i - self.hi + 1} double(s) past its end"
        return f"{bad.size} guard value(s) of {self.name} overwritten; first {where}: {s[i]:#018x}"


# ---- data and references -------------------------------------------------------------------------------------------------
class Refs:
    """a data set with NC right-hand sides per side and their exact products, computed once; the CSR of A and of A'"""
    def __init__(self, d, nc=NC, ata_cols=3):
        self.d, self.nc = d, nc
        self.inp = (d.X(nc), d.U(nc))
        self.out = (d.Y(nc), d.Z(nc))
        self.n_in, self.n_out = (d.ncol, d.nrow), (d.nrow, d.ncol)
        order = np.argsort(d.cols, kind="stable")           # A': stably column-ordered, every row of A' in ascending A-row order
        t_rp = np.zeros(d.ncol + 1, np.int32)
        np.cumsum(np.bincount(d.cols, minlength=d.ncol), out=t_rp[1:])
        self.csr = ((d.rp, d.cols, d.vals), (t_rp, d.rows[order], None if d.vals is None else d.vals[order]))
        self.ata = []
        for j in range(ata_cols):                           # A'A x is exact only on some sets: exact_sum says on which
            try:
                self.ata.append(E.ata(d.nrow, d.ncol, d.rows, d.cols, d.vals, self.inp[0][:, j]))
            except AssertionError:
                self.ata = []
                break

    def run(self, what, side, j0, k):
        a = (self.inp if what == "in" else self.out)[side]
        return np.ascontiguousarray(a[:, j0:j0 + k]).reshape(-1)


class _Sets(dict):
    """name -> Data of the small sets the walks run on, each built on first use"""
    MAKE = {"wide_range": E.wide_range, "wide_range_odd": E.wide_range_odd,
            "long_rows_heavy": lambda: E.long_rows(profile="heavy", nrow=4000, seed=6), "subnormal": E.subnormal, "zeros": E.zeros,
            "subnormal_pattern": E.subnormal_pattern, "zeros_pattern": lambda: E.zeros(valued=False),
            "long_rows_single_pattern": lambda: E.long_rows(valued=False, seed=7)}

    def __missing__(self, name):
        d = self[name] = self.MAKE[name]()
        assert d.name == name
        return d


_SETS = _Sets()
SET_NAMES = list(_Sets.MAKE)
# the sets the GPU walks run on.  All eight at 150 steps and two seeds per (set, copy) take about 27 s on the MI355X, two of them 11 s,
# tests/test_gpu_exact.py 9.3 s, and tests/test_gpu_lifecycle.py is to stay below that: steps and seeds are at their floor, so sets
# go.  Kept: the odd-sized set (vectors of odd length, slices without LDS DMA: where a stray load or store is most likely); every
# walk also runs pattern-only handles of its set.  The stand-in (tests/test_lifecycle_model.py) still walks all eight.
GPU_SET_NAMES = ["wide_range_odd"]


def data_sets():
    return _SETS


_REFS = {}


def refs_of(d, nc=NC, ata_cols=3):
    key = (d.name, d.nrow, d.ncol, d.nnz, nc)
    if key not in _REFS:
        _REFS[key] = Refs(d, nc, ata_cols)
    return _REFS[key]


def mid_size():
    """about 140 000 x 40 000, three column bands: with bin_rows / tile_rows of 32 it has more generations of resident workgroups
    than the largest nparts of a walk (12), so its products in parts are really cut"""
    return E.wide_range(seed=21, nrow=140000, ncol=40000, name="wide_range_mid")


# ---- the systems of the solver pairs and the models of their solves -----------------------------------------------------------
class PairSystem:
    """a system of _cg_model with the CSR of A and of A' as the pair's two handles hold them, the products the models run on
    (exact bincounts for the exact family, the oracle's storage-order sums for the general system) and, per handle, a Data with
    integer-valued vectors for the walk's products"""
    def __init__(self, kind, valued=False):
        self.kind = kind
        if kind == "exact":
            self.fam = M.exact_family(valued)
            self.s = self.fam.s
            self.a_csr, self.t_csr = self.fam.a_csr(), self.fam.t_csr()
            self.products = self.fam.products()
        else:
            self.fam = None
            self.s = M.systems(large=False)["binary_F257"]
            self.a_csr, self.t_csr = self.s.a_csr(), self.s.t_csr_coo()
            self.products = M.csr_products(self.s.nrow, self.s.ncol, self.a_csr, self.t_csr)
        self.name = self.s.name
        self.data = tuple(self._data(side) for side in (0, 1))

    def _data(self, side):
        rp, cc, vv = (self.a_csr, self.t_csr)[side]
        nrow, ncol = (self.s.nrow, self.s.ncol) if side == 0 else (self.s.ncol, self.s.nrow)
        rng = np.random.default_rng([31, side, zlib.crc32(self.name.encode())])
        ints = lambda n: rng.integers(-512, 513, n).astype(np.float64)
        cols = [ints(ncol) for _ in range(NC)]
        d = E.Data(f"{self.name}_{'At' if side else 'A'}", nrow, ncol, np.repeat(np.arange(nrow), np.diff(rp)), cc, vv, cols[0], ints(nrow),
                   lambda j: cols[j])
        d.system = self
        return d


_PAIR_SYSTEMS = {}


def pair_system(kind, valued=False):
    key = (kind, bool(valued) and kind == "exact")
    if key not in _PAIR_SYSTEMS:
        _PAIR_SYSTEMS[key] = PairSystem(*key)
    return _PAIR_SYSTEMS[key]


Solved = collections.namedtuple("Solved", "x iters infos state extra")     # x: (F,), (F, k) or (m, F); extra: shifts / columns
_SOLVED = {}


def _key(a):
    return None if a is None else hash(np.ascontiguousarray(a, np.float64).tobytes())


def solve_model(ps, solver, b, lam, tol, max_iter=0, precond=P.PRECOND_NONE, x0=None, diag=None, lams=None, tree="device"):
    """the model's solve (tests/_cg_model.py, _pcg_model.py, _mscg_model.py, _pcgn_model.py) of a pair's system; kept by its
    arguments: the walk and the stand-in ask for the same solves again and again"""
    F = ps.s.ncol
    key = (ps.name, solver, _key(b), float(lam), float(tol), max_iter, precond, _key(x0), _key(diag), None if lams is None else tuple(lams), tree)
    if key in _SOLVED:
        return _SOLVED[key]
    am, atm, am2, atm2 = ps.products
    dinv = None
    if precond == P.PRECOND_JACOBI:
        dinv = P.dinv_of(P.gram_diag(ps.t_csr, lam))
    elif precond == P.PRECOND_DIAG:
        dinv = P.dinv_of(diag)
    if solver == "cg":
        r = M.cg(F, am, atm, b, lam, tol, tree)
        out = Solved(r.x, [r.iterations], None, r.state, None)
    elif solver == "cg2":
        r = M.cg2(F, am2, atm2, np.asarray(b).reshape(F, 2), lam, tol, tree)
        out = Solved(r.x, [r.iterations], None, r.state, None)
    elif solver == "pcg":
        r = P.pcg(F, am, atm, b, lam, tol, max_iter, dinv, x0, tree)
        out = Solved(r.x, [r.iterations], [N.info_of(r)], r.state, None)
    elif solver == "mscg":
        r = S.mscg(F, am, atm, b, lams, tol, max_iter, tree)
        out = Solved(r.X, [i.iterations for i in r.infos], list(r.infos), r.state, r.shifts)
    elif solver == "mscgn":                                   # column j IS fs_mscg on B[:, j] (tests/_mscgn_model.py)
        B = np.asarray(b, np.float64).reshape(F, -1)
        cols = [solve_model(ps, "mscg", np.ascontiguousarray(B[:, j]), lam, tol, max_iter, lams=lams, tree=tree) for j in range(B.shape[1])]
        pairs = [(i, j) for i in range(len(lams)) for j in range(B.shape[1])]          # info[i * k + j]
        out = Solved(np.stack([c.x for c in cols], 2), [cols[j].iters[i] for i, j in pairs], [cols[j].infos[i] for i, j in pairs],
                     cols[0].state, [(c.state, c.extra) for c in cols])
    else:                                                     # fs_pcgn; fs_pcgn_lambdas: column j IS fs_pcg at lams[j]
        B = np.asarray(b, np.float64).reshape(F, -1)
        lam_of = (lambda j: lam) if solver == "pcgn" else (lambda j: lams[j])
        cols = [solve_model(ps, "pcg", np.ascontiguousarray(B[:, j]), lam_of(j), tol, max_iter, precond,
                            None if x0 is None else np.ascontiguousarray(np.asarray(x0).reshape(F, -1)[:, j]), diag, None, tree)
                for j in range(B.shape[1])]
        out = Solved(np.stack([c.x for c in cols], 1), [c.iters[0] for c in cols], [c.infos[0] for c in cols], cols[0].state,
                     [c.state for c in cols])
    _SOLVED[key] = out
    return out


def exact_cases(fam):
    """every solve the walk runs on the exact family: (solver, what, keyword arguments of solve_model)"""
    s = fam.s
    out = [("cg", "fs_cg", dict(b=s.b)), ("cg2", "fs_cg2", dict(b=fam.B2.reshape(-1)))]
    for pname, precond in (("none", P.PRECOND_NONE), ("jacobi", P.PRECOND_JACOBI), ("diag", P.PRECOND_DIAG)):
        diag = fam.diag if precond == P.PRECOND_DIAG else None
        for start in ("cold", "exact", "other", "b = 0"):
            b = np.zeros(fam.F) if start == "b = 0" else s.b
            x0 = fam.x0(s.b, start) if start in ("exact", "other") else None
            out.append(("pcg", f"fs_pcg {pname} {start}", dict(b=b, precond=precond, diag=diag, x0=x0)))
        for k in PCGN_KS:
            B = fam.panel(k)
            for start in ("cold", "mixed"):
                out.append(("pcgn", f"fs_pcgn k {k} {pname} {start}",
                            dict(b=B.reshape(-1), precond=precond, diag=diag, x0=fam.x0(B, "mixed").reshape(-1) if start == "mixed" else None)))
    for name, lams in fam.ladders.items():
        out.append(("mscg", f"fs_mscg {name}", dict(b=s.b, lams=list(lams))))
    # fs_pcgn_lambdas: a lambda per column, every d + lambda_j a power of two (the rungs of the ladders of 3 and 16, duplicates included), so
    # column j is x = b_j / (d + lambda_j) at iteration 0 like fs_pcg; a zero column (panel: column k // 2); warm columns that take
    # turns -- exact, 2 x exact (r = -b: one pass), cold
    for pname, precond in (("none", P.PRECOND_NONE), ("jacobi", P.PRECOND_JACOBI), ("diag", P.PRECOND_DIAG)):
        for k in PCGN_KS:
            B = fam.panel(k)
            rungs = fam.ladders["m3"] + fam.ladders["m16"]
            lams = [rungs[j % len(rungs)] for j in range(k)]
            X0 = np.zeros(B.shape)
            for j in range(k):
                X0[:, j] = B[:, j] * ((1.0, 2.0, 0.0)[j % 3] / (fam.d + lams[j]))
            for start in ("cold", "mixed"):
                out.append(("pcgn_lambdas", f"fs_pcgn_lambdas k {k} {pname} {start}",
                            dict(b=B.reshape(-1), precond=precond, diag=fam.diag if precond == P.PRECOND_DIAG else None, lams=lams,
                                 x0=X0.reshape(-1) if start == "mixed" else None)))
    # fs_mscgn: the ladders of 1, 3 and 8 lambdas (the smallest twice, another rung twice) for k right-hand sides
    ladders = {"m1": fam.ladders["m1"], "m3": fam.ladders["m3"], "m8": fam.ladders["m16"][:8]}
    for k in MSCGN_KS:
        for name, lams in ladders.items():
            out.append(("mscgn", f"fs_mscgn k {k} {name}", dict(b=fam.panel(k).reshape(-1), lams=list(lams))))
    return out


_STRICT = {}


def strict_cases(ps):
    if ps.name not in _STRICT:
        _STRICT[ps.name] = _strict_cases(ps)
    return _STRICT[ps.name]


def _strict_cases(ps):
    """the solves under strict_order on the general system: caps of at most 12, so that columns and shifts freeze at different
    iterations or meet the cap; fs_cg at a tol its model meets within about 20 iterations"""
    s = ps.s
    i = np.arange(s.ncol, dtype=np.float64)
    B5 = np.stack([s.b, s.b, np.zeros(s.ncol), s.b * 1.5 + np.sin(i * 0.22 + 0.6), np.cos(i * 0.05) * 1e-3], 1)
    X3 = np.stack([0.25 * np.sin(i * 0.37 + 0.2), np.zeros(s.ncol), 0.125 * np.cos(i * 0.11)], 1)
    dg = P.gram_diag(ps.t_csr, s.lam) * (1.0 + 0.5 * np.cos(i * 1.7)) + 0.125
    # warm columns that freeze at different iterations: cold, four iterations in, zero, done before the first product, cold
    X5 = np.zeros(B5.shape)
    X5[:, 1] = solve_model(ps, "pcg", s.b, s.lam, 1e-4, 4, P.PRECOND_JACOBI).x
    X5[:, 3] = solve_model(ps, "pcg", np.ascontiguousarray(B5[:, 3]), s.lam, 1e-6, 0, P.PRECOND_JACOBI).x
    return [("cg", "fs_cg", dict(b=s.b, tol=1e-4)),
            ("pcg", "fs_pcg jacobi cap 12", dict(b=s.b, precond=P.PRECOND_JACOBI, max_iter=12, tol=s.tol)),
            ("pcg", "fs_pcg none warm cap 5", dict(b=s.b, x0=X3[:, 0], max_iter=5, tol=s.tol)),
            ("mscg", "fs_mscg ladder of 8 cap 12", dict(b=s.b, lams=[s.lam * f for f in (1e3, 10.0, 1e6, 1.0, 30.0, 1e4, 3.0, 1.0)], max_iter=12, tol=1e-6)),
            ("pcgn", "fs_pcgn k 5 jacobi warm cap 12", dict(b=B5.reshape(-1), precond=P.PRECOND_JACOBI, x0=X5.reshape(-1), max_iter=12, tol=1e-4)),
            ("pcgn", "fs_pcgn k 3 diag warm cap 4", dict(b=np.ascontiguousarray(B5[:, 2:5]).reshape(-1), precond=P.PRECOND_DIAG, diag=dg,
                                                         x0=X3.reshape(-1), max_iter=4, tol=s.tol)),
            # (the lambdas: the system's own where X5 holds that lambda's iterates, so that the warm columns freeze as in fs_pcgn)
            ("pcgn_lambdas", "fs_pcgn_lambdas k 5 jacobi warm cap 12",
             dict(b=B5.reshape(-1), precond=P.PRECOND_JACOBI, x0=X5.reshape(-1), max_iter=12, tol=1e-4, lams=[s.lam * 30.0, s.lam, s.lam, s.lam, s.lam * 1e3])),
            ("pcgn_lambdas", "fs_pcgn_lambdas k 3 diag cap 4",
             dict(b=np.ascontiguousarray(B5[:, 2:5]).reshape(-1), precond=P.PRECOND_DIAG, diag=dg, x0=X3.reshape(-1), max_iter=4, tol=s.tol,
                  lams=[s.lam, s.lam * 10.0, s.lam])),
            ("mscgn", "fs_mscgn k 3 ladder of 8 cap 12",
             dict(b=np.ascontiguousarray(B5[:, (0, 2, 3)]).reshape(-1), lams=[s.lam * f for f in (1e3, 10.0, 1e6, 1.0, 30.0, 1e4, 3.0, 1.0)], max_iter=12, tol=1e-6)),
            ("mscgn", "fs_mscgn k 1 m 3", dict(b=s.b, lams=[s.lam * 3.0, s.lam, s.lam], max_iter=12, tol=1e-6))]


def repacking_cases(ps):
    """the solves of exact_cases (exact family) or strict_cases (general system) that narrow under option "pcgn_compact" when every
    rung is usable, as (solver, index among that solver's exact cases / among the strict cases, what): Jacobi panels of 2, 3, 5
    and 17 columns whose zero and converged columns freeze at the start; the k = 5 solves whose columns freeze at different
    iterations.  tests/test_lifecycle_model.py holds each against the plan model"""
    if ps.fam is None:
        return [(sv, i, what) for i, (sv, what, kw) in enumerate(strict_cases(ps)) if sv in NARROWING and kw["b"].size // ps.s.ncol == 5]
    out = []
    for solver in NARROWING:
        cases = [c for c in exact_cases(ps.fam) if c[0] == solver]
        out += [(solver, j, what) for j, (_, what, kw) in enumerate(cases) if kw["b"].size // ps.fam.F in (2, 3, 5, 17) and "jacobi" in what
                and "k 2 jacobi mixed" not in what]              # (both columns frozen at the start: done before the first iteration)
    return out


def work_space(solver, F, Nrow, k=1, pre=False, nslots=0, widths=()):
    """the doubles of every device buffer a solve asks for, one entry per allocation of fs_cg.hip (SolveFrame::alloc and the callers'
    own blocks): r, p, q (k F each), tmp (k N), the partial sums kRedBlocks * 3, the sums, st[]; F for dinv / s; fs_mscg: one
    block of ((F + 1) & ~1) nslots directions and its per-shift scalars; fs_pcgn, fs_pcgn_lambdas: one block of 2048 k partials and 512
    scalars; fs_mscgn: one block of ((F k + 1) & ~1) nslots direction panels, one of 2048 k partials and 9344 scalars; narrowing
    (widths: the two widest usable widths below k, w1 > w2, w2 = 0 when there is one): X, R, P at w1, X at w2 and 512 scalars.
    tests/test_lifecycle_model.py holds the sums against the header's formulas ("Work space per solve")"""
    out = [k * F, k * F, k * F, k * Nrow, M.RED_BLOCKS * 3, 4, M.CG_STATE_DOUBLES]
    if pre:
        out.append(F)
    if solver == "mscg":
        out += [((F + 1) & ~1) * nslots, S.MAX_SHIFTS * S.MS_STRIDE]
    if solver in ("pcgn", "pcgn_lambdas"):
        out.append(2 * M.RED_BLOCKS * k + N.MAX_RHS * N.PN_STRIDE)
    if solver == "mscgn":
        out += [((F * k + 1) & ~1) * nslots, 2 * M.RED_BLOCKS * k + MSCGN_SCALARS]
    if widths:
        w1, w2 = widths
        out += [w1 * F] * 3 + [w2 * F, N.MAX_RHS * N.PN_STRIDE]
    return [n for n in out if n > 0]


# ---- the model of a handle -----------------------------------------------------------------------------------------------
class Model:
    """what include/fastsparse_hip.h promises about one handle, from the calls made on it"""
    def __init__(self, has_t):
        self.has_t = has_t
        self.released = [False, False]
        self.kept = [1, 1]              # fs_matrix_spmv_kernel under default options: >= 6 = a re-ordered copy is kept
        self.orderable = [True, True]   # (LDS-staged copy) fixed-order sums possible
        self.ldsx_shared = [False, False]
        self.prepared = [set(), set()]

    def choice(self, side, o):
        """fs_matrix_spmv_kernel under the options o (fs_abi.hip: spmv_choice)"""
        kept, sk = self.kept[side], o["spmv_kernel"]
        if not o["strict_order"] and kept >= 6 and sk in (0, kept) and (kept != 8 or not o["reproducible"] or self.orderable[side]):
            return kept
        return 2 if sk == 2 else 1

    def product(self, side, o):
        """status of a single-vector product (device or host vectors, whole or part 0 of a product in parts)"""
        if side and not self.has_t:
            return FS_ERR_NO_TRANSPOSE
        return FS_ERR_RELEASED if self.released[side] and self.choice(side, o) < 6 else FS_OK

    def multi(self, side, plan):
        """status of a k-column product that the library says it runs on `plan`"""
        if side and not self.has_t:
            return FS_ERR_NO_TRANSPOSE
        return FS_ERR_RELEASED if self.released[side] and plan in (ROW_PLAN, MFMA_PLAN) else FS_OK

    def ata(self, o):
        """(status, builds A'): the fused kernel runs on an LDS-staged copy with one chunk per panel or on the plain CSR; the two
        products build A' on first use, from the plain CSR"""
        if o["ata_kernel"] == 2 and not o["strict_order"] and not o["reproducible"]:
            on_copy = self.kept[0] == 8 and not self.ldsx_shared[0]
            return (FS_ERR_RELEASED if self.released[0] and not on_copy else FS_OK), False
        builds = not self.has_t
        if builds and self.released[0]:
            return FS_ERR_RELEASED, False
        if self.released[0] and self.choice(0, o) < 6:
            return FS_ERR_RELEASED, builds
        return None, builds             # then the status of the A' product, known once A' exists

    def prepare_refused(self, side, needs):
        """fs_matrix_prepare answers FS_ERR_RELEASED: one-time work that reads the plain arrays (fs_debug_spmm_needs bits 0, 1) is
        left and the side gave them back"""
        return self.released[side] and bool(needs & 3)

    def width_usable(self, side, w, needs, plan, o):
        """option "pcgn_compact": a side lets a solve narrow to w columns -- its prepare(w) is not refused (needs: before the
        solve) and the product of w columns (plan: what fs_matrix_spmm_plan says after the solve's own prepare; w = 1: the
        single-vector product) does not read plain arrays that were given back"""
        if w == 1:
            return self.product(side, o) == FS_OK
        return not self.prepare_refused(side, needs) and self.multi(side, plan) == FS_OK

    def release_csr(self):
        sides = [s for s in (0, 1) if (s == 0 or self.has_t) and self.kept[s] >= 6 and not self.released[s]]
        for s in sides:
            self.released[s] = True
        return len(sides)

    def all_released(self):
        return self.released[0] and (not self.has_t or self.released[1])


# ---- the walk ------------------------------------------------------------------------------------------------------------
def _rc(exc):
    m = re.search(r"failed \((-?\d+)\)", str(exc))
    assert m, f"an error without a status: {exc!r}"
    return int(m.group(1))


class Handle:
    def __init__(self, name, refs, copy, borrow):
        self.name, self.refs, self.copy, self.borrow = name, refs, copy, borrow
        self.A = None
        self.model = None
        self.vec = {}
        self.arrays = {}                # guarded CSR arrays of a borrowed matrix: (side, which) -> Guarded
        self.array_consts = {}
        self.nparts_seen = set()
        self.base_bytes = None
        self.prove = False              # the last call was refused: the next product must be exact
        self.pair = None                # the solver pair this handle is half of


class Pair:
    """a solver pair: the handle of A and the handle of A', two separate handles as fs_cg takes them"""
    def __init__(self, ps, HA, HT):
        self.ps, self.A, self.At = ps, HA, HT
        self.saved_diag = None          # the d of the last successful fs_gram_diag(At, the system's lambda)


class Walk:
    def __init__(self, backend, data, copy, seed, steps=150, upto=None, copies=None, kmax=17, nc=NC, nhandles=3, ata_cols=3, solvers=True):
        self.b, self.data, self.copy, self.seed, self.solvers = backend, data, copy, seed, solvers
        self.steps = steps if upto is None else min(steps, upto)
        self.rng = np.random.default_rng([seed, zlib.crc32(f"{data.name}/{copy}".encode())])     # every (set, copy) walks its own way
        self.copies = list(copies or backend.copies())
        self.ks = tuple(k for k in KS if k <= kmax)
        self.kmax, self.nc, self.nhandles, self.ata_cols = max(self.ks), nc, nhandles, ata_cols
        self.log, self.step = [], -1
        self.handles = []
        self.made = 0
        self.o = {}                     # the flippable options as the walk has set them
        self.neutral = {}
        self.counts = {"ops": {}, "status": {}, "k": [set(), set()], "nparts": {}, "host_behind_device": 0, "restore": set(),
                       "recovered": 0, "part_between": 0, "poison_seen": 0, "poison_probed": 0, "poisoned": 0, "repacked": 0, "solves": {},
                       "solver_status": {}}
        self.pairs = []

    # -- bookkeeping ----
    def fail(self, kind, msg):
        tail = "\n    ".join(self.log[-20:])
        raise WalkFailure(f"{kind}: {msg}\n  data set {self.data.name}, copy {self.copy!r}, seed {self.seed}, step {self.step} "
                          f"(replay: run_walk(..., upto={self.step + 1}))\n  last operations:\n    {tail}", self.step, kind)

    def note(self, text):
        self.log.append(f"{self.step:4d} {text}")

    def count(self, op):
        self.counts["ops"][op] = self.counts["ops"].get(op, 0) + 1

    def call(self, f, *a, **kw):
        """status of a library call (the bindings raise on a negative status, with the status in the message)"""
        try:
            r = f(*a, **kw)
        except self.b.Error as ex:
            return _rc(ex), None
        return FS_OK, r

    def expect(self, H, what, rc, want):
        self.counts["status"][want] = self.counts["status"].get(want, 0) + 1
        self.log[-1] += f" -> {STATUS_NAMES.get(rc, rc)}"
        if rc != want:
            self.fail("status", f"{what} on {H.name} returned {STATUS_NAMES.get(rc, rc)}, the header promises "
                      f"{STATUS_NAMES.get(want, want)} (model: released {H.model.released}, has A' {H.model.has_t}, kept {H.model.kept}, "
                      f"options {self.o})")
        if rc != FS_OK:
            H.prove = True

    # -- handles ----
    def create(self, first=False, with_t=None, borrow=None, data=None):
        i = self.made
        self.made += 1
        d = self.data if data is None else data
        if first:
            copy, pattern = self.copy, False
        elif data is not None:              # half of a solver pair: any copy the builder makes of it, no built transpose
            copy, pattern, with_t = self.copies[int(self.rng.integers(len(self.copies)))], False, False
        else:
            copy = self.copies[int(self.rng.integers(len(self.copies)))]
            pattern = i == 1 or bool(self.rng.integers(3) == 0)      # at least one handle of every walk is pattern-only
        if pattern and d.vals is not None:
            d = d.pattern()
        draw = (bool(self.rng.integers(2)), bool(self.rng.integers(3)))
        borrow, with_t = draw[0] if borrow is None else borrow, draw[1] if with_t is None else with_t
        H = Handle(f"h{i}[{d.name}/{copy}{'/borrowed' if borrow else ''}]", refs_of(d, self.nc, self.ata_cols), copy, borrow)
        r = H.refs
        n = max(d.nrow, d.ncol) * self.kmax
        for role in ("in", "out"):
            H.vec[role] = Guarded(self.b.mem, f"{role} vector of {H.name}", n)
            H.vec["host " + role] = Guarded(self.b.hostmem, f"host {role} vector of {H.name}", max(d.nrow, d.ncol))
        H.vec["tmp"] = Guarded(self.b.mem, f"tmp of {H.name}", d.nrow)
        arrays = self.arrays_for(H, 0) if borrow else r.csr[0]
        with self.b.options(**self.neutral), self.b.options(**self.b.creation_options(copy)):
            H.A = self.b.create(d, copy, arrays, borrow, must=data is None)
            H.model = Model(False)
            self.learn_side(H, 0)
            if with_t:
                rc, _ = self.call(H.A.build_transpose, self.b.stream())
                if rc != FS_OK:
                    self.fail("status", f"build_transpose at creation of {H.name} returned {rc}")
                H.model.has_t = True
                self.learn_side(H, 1)
        H.base_bytes = H.A.device_bytes()
        self.handles.append(H)
        self.note(f"create {H.name} kept {H.model.kept} A' {with_t}")
        return H

    def arrays_for(self, H, side):
        """the CSR of a side in guarded device arrays (int arrays in allocations of doubles, 16-byte aligned: they are borrowed)"""
        mem = self.b.mem
        out = []
        for which, a in zip(("row_ptr", "cols", "vals"), H.refs.csr[side]):
            if a is None:
                out.append(None)
                continue
            nd = a.size if a.dtype == np.float64 else (a.size + 1) // 2
            g = Guarded(mem, f"{which} of {'A' + chr(39) if side else 'A'} of {H.name}", nd)
            v = g.place(nd, 0)
            if a.dtype == np.float64:
                mem.put(v, a)
                view = v
            else:
                view = mem.i32(v)[:a.size]
                mem.put(view, a)
                if a.size & 1:
                    mem.put(mem.i32(v)[a.size:], np.zeros(1, np.int32))
            H.arrays[(side, which)] = g
            H.array_consts[(side, which)] = (view, mem.const(a))
            out.append(view)
        return tuple(out)

    def learn_side(self, H, side):
        """what the model cannot know from the calls: which copy the builder kept (under default options)"""
        m = H.model
        m.kept[side] = self.b.kernel_code(H.A, side)
        m.orderable[side] = self.b.ldsx_orderable(H.A, side) != 0
        m.ldsx_shared[side] = bool(self.b.tiled_layout(H.A, side) & 2) if m.kept[side] == 8 else False

    def destroy(self, H):
        H.A.close()
        self.handles.remove(H)

    # -- checks after every operation ----
    def check_all(self, H, ins=(), outs=()):
        """guards of every vector of every handle; inputs unchanged; outputs exact (all bit for bit, where the vectors live)"""
        every = [g for h in self.handles for g in list(h.vec.values()) + list(h.arrays.values())]
        for mem in [self.b.mem] + ([self.b.hostmem] if self.b.hostmem is not self.b.mem else []):
            g = mem.first_bad_guard([g for g in every if g.mem is mem])
            if g is not None:
                self.fail("guard", g.first_broken())
        for h in self.handles:
            for key, (view, const) in h.array_consts.items():
                if not self.b.mem.eq(view, const):
                    self.fail("input modified", f"{key[1]} of side {key[0]} of borrowed {h.name} changed")
        for g, want, what in ins:
            if not g.mem.eq(g.view, g.mem.const(want)):
                self.fail("input modified", f"{g.name} ({what}): {E.first_mismatch(g.mem.get(g.view), want)}")
        for g, want, what in outs:
            if not g.mem.eq(g.view, g.mem.const(want)):
                self.wrong(g, g.mem.get(g.view), want, what)

    def wrong(self, g, got, want, what, kind="not exact"):
        msg = f"{g.name} ({what}): {E.first_mismatch(got, want)}"
        nan = np.flatnonzero(np.isnan(got))
        for i in nan[:64]:
            tag = guard_tag(got.view(np.int64)[i])
            if tag is not None:
                self.fail("guard value read", f"a guard value of {TAGS.get(tag, tag)} reached element {int(i)} of the sum; " + msg)
        if nan.size and (got.view(np.int64)[nan] == PREFILLS["nan"]).any():
            msg += f"; {int((got.view(np.int64) == PREFILLS['nan']).sum())} element(s) still hold the prefill"
        self.fail(kind, msg)

    def bookkeeping(self, H):
        m = H.model
        if bool(self.b.has_transpose(H.A)) != m.has_t:
            self.fail("bookkeeping", f"fs_matrix_has_transpose of {H.name} is {self.b.has_transpose(H.A)}, model {m.has_t}")
        for side in (0, 1) if m.has_t else (0,):
            got, want = self.b.kernel_code(H.A, side), m.choice(side, self.o)
            if got != want:
                self.fail("bookkeeping", f"fs_matrix_spmv_kernel({H.name}, {side}) = {got}, the model of spmv_choice says {want} "
                          f"(kept {m.kept}, options {self.o})")

    # -- vectors of one product ----
    def place_in(self, H, role, side, j0, k):
        g = H.vec[role]
        want = H.refs.run("in", side, j0, k)
        g.mem.put(g.place(want.size, int(self.rng.integers(2))), want)
        return g, want

    def place_out(self, H, role, side, k):
        g = H.vec[role]
        fill = ("nan", "-0.0")[int(self.rng.integers(4) == 0)]
        g.mem.fill_bits(g.place(H.refs.n_out[side] * k, int(self.rng.integers(2))), PREFILLS[fill])
        g.prefill = PREFILLS[fill]
        return g

    def columns(self, k):
        return int(self.rng.integers(self.nc - k + 1))

    # -- operations ----
    def op_spmv(self, H, side, host=False):
        j = self.columns(1)
        pre = "host " if host else ""
        gi, wi = self.place_in(H, pre + "in", side, j, 1)
        go = self.place_out(H, pre + "out", side, 1)
        want = H.model.product(side, self.o)
        self.note(f"{H.name} {'spmv_host' if host else 'spmv'} side {side} column {j}")
        if host:
            rc, _ = self.call(H.A.spmv_host, go.view, gi.view, transposed=bool(side))
        else:
            rc, _ = self.call(H.A.spmv, go.view, gi.view, self.b.stream(), transposed=bool(side))
        self.expect(H, "a single-vector product", rc, want)
        self.check_all(H, [(gi, wi, "x")], [(go, H.refs.run("out", side, j, 1), f"side {side} column {j}")] if rc == FS_OK else [])
        return rc

    def op_dev_then_host(self, H):
        """a host-vector product directly behind a device-vector product on the OTHER stream, nothing in between: legal, the library
        orders it behind the handle's last product (they share the handle's scratch)"""
        self.b.switch_stream()
        s1, s2 = int(self.rng.integers(2)), int(self.rng.integers(2))
        j1, j2 = self.columns(1), self.columns(1)
        gi, wi = self.place_in(H, "in", s1, j1, 1)
        go = self.place_out(H, "out", s1, 1)
        hi, whi = self.place_in(H, "host in", s2, j2, 1)
        ho = self.place_out(H, "host out", s2, 1)
        w1, w2 = H.model.product(s1, self.o), H.model.product(s2, self.o)
        self.note(f"{H.name} spmv side {s1} column {j1} on stream {self.b.stream_index()}, then spmv_host side {s2} column {j2}")
        rc1, _ = self.call(H.A.spmv, go.view, gi.view, self.b.stream(), transposed=bool(s1))
        rc2, _ = self.call(H.A.spmv_host, ho.view, hi.view, transposed=bool(s2))
        self.expect(H, "the device-vector product", rc1, w1)
        self.expect(H, "the host-vector product behind it", rc2, w2)
        outs = [(go, H.refs.run("out", s1, j1, 1), "device vectors")] if rc1 == FS_OK else []
        outs += [(ho, H.refs.run("out", s2, j2, 1), "host vectors behind a device-vector product")] if rc2 == FS_OK else []
        self.check_all(H, [(gi, wi, "x"), (hi, whi, "host x")], outs)
        if rc1 == FS_OK and rc2 == FS_OK:
            self.counts["host_behind_device"] += 1

    def op_spmm(self, H, side):
        k = int(self.rng.choice(self.ks))
        j0 = self.columns(k)
        gi, wi = self.place_in(H, "in", side, j0, k)
        go = self.place_out(H, "out", side, k)
        m = H.model
        plan = self.b.spmm_plan(H.A, k, side) if (not side or m.has_t) else None
        want = m.multi(side, plan)
        self.b.last_spmm_plan()
        self.note(f"{H.name} spmm side {side} k {k} columns {j0}.. plan {plan}")
        rc, _ = self.call(H.A.spmm, go.view, gi.view, k, self.b.stream(), transposed=bool(side))
        self.expect(H, f"a {k}-column product", rc, want)
        if plan is not None:
            ran = self.b.last_spmm_plan()
            if ran != plan:
                self.fail("bookkeeping", f"fs_matrix_spmm_plan({H.name}, {k}, {side}) said {plan}, fs_debug_last_spmm_plan says {ran} ran")
        self.counts["k"][side].add(k)
        self.check_all(H, [(gi, wi, "X")], [(go, H.refs.run("out", side, j0, k), f"side {side} k {k} columns {j0}.. plan {plan}")] if rc == FS_OK else [])

    def op_ata(self, H):
        ak = int(self.rng.choice((0, 2)))
        j = int(self.rng.integers(len(H.refs.ata)))
        m = H.model
        with self.b.options(ata_kernel=ak):
            o = dict(self.o, ata_kernel=ak)
            gi, wi = self.place_in(H, "in", 0, j, 1)
            go = self.place_out(H, "out", 1, 1)
            gt = H.vec["tmp"]
            self.b.mem.fill_bits(gt.place(H.refs.d.nrow, int(self.rng.integers(2))), PREFILLS["nan"])
            want, builds = m.ata(o)
            self.note(f"{H.name} ata ata_kernel {ak} column {j}")
            rc, _ = self.call(H.A.ata, go.view, gi.view, gt.view, self.b.stream())
            if builds:                                    # A' was built inside the call, under the options of the moment
                m.has_t = True
                self.learn_neutral(H, 1)
                H.base_bytes = H.A.device_bytes()
                if want is None:
                    want = m.product(1, o)
            elif want is None:
                want = m.product(1, o)
            self.expect(H, "fs_ata_mul", rc, want)
        self.check_all(H, [(gi, wi, "x")], [(go, H.refs.ata[j], f"A'A x, ata_kernel {ak}, column {j}")] if rc == FS_OK else [])

    def learn_neutral(self, H, side):
        with self.b.options(**self.neutral):
            self.learn_side(H, side)

    def between_parts(self, H):
        """between the parts of one product the walk may run products on OTHER handles -- never on the same one: the header leaves
        that undefined (the parts share the handle's scratch)"""
        others = [h for h in self.handles if h is not H]
        if others and self.rng.integers(3) == 0:
            self.counts["part_between"] += 1
            self.op_spmv(others[int(self.rng.integers(len(others)))], 0)

    def op_part(self, H, side, k):
        """the product in nparts parts, all parts in order; a single-vector op runs three such products with nparts of their own, so
        that one side of a handle meets more than eight (nparts, kernel) pairs and early ones come back after their plan is gone"""
        for _ in range(3 if k == 1 else 1):
            rc = self.one_product_in_parts(H, side, k, int(self.rng.integers(1, 13)))
            if rc != FS_OK:
                break

    def one_product_in_parts(self, H, side, k, nparts):
        j0 = self.columns(k)
        m = H.model
        gi, wi = self.place_in(H, "in", side, j0, k)
        go = self.place_out(H, "out", side, k)
        ok_side = not side or m.has_t
        if k == 1:
            want = m.product(side, self.o)
            if want == FS_OK:
                H.nparts_seen.add((side, nparts, m.choice(side, self.o)))
                self.counts["nparts"][H.name] = max(len({t for t in H.nparts_seen if t[0] == s}) for s in (0, 1))
        else:
            want = m.multi(side, self.b.spmm_plan(H.A, k, side) if ok_side else None)
        self.note(f"{H.name} {'spmv' if k == 1 else 'spmm'}_part side {side} k {k} nparts {nparts} columns {j0}..")
        rc, rows = self.call(H.A.part_rows, nparts, bool(side), k)
        if not ok_side:
            self.expect(H, "fs_spmm_part_rows", rc, FS_ERR_NO_TRANSPOSE)
            self.check_all(H, [(gi, wi, "x")])
            return rc
        if rc != FS_OK:
            self.fail("status", f"fs_spmm_part_rows({H.name}, {side}, {k}, {nparts}) returned {rc}")
        n = H.refs.n_out[side]
        if rows[0] != 0 or rows[-1] != n or any(a > b for a, b in zip(rows, rows[1:])):
            self.fail("part rows", f"cuts of {H.name} side {side} nparts {nparts}: {rows}")
        full = H.refs.run("out", side, j0, k)
        for p in range(nparts):
            rc, _ = (self.call(H.A.spmv_part, go.view, gi.view, p, nparts, self.b.stream(), transposed=bool(side)) if k == 1 else
                     self.call(H.A.spmm_part, go.view, gi.view, k, p, nparts, self.b.stream(), transposed=bool(side)))
            if p == 0 or rc != FS_OK:
                self.expect(H, f"part {p} of {nparts}", rc, want)
                if rc != FS_OK:
                    break
            if not gi.mem.eq(gi.view, gi.mem.const(wi)):
                self.fail("input modified", f"{gi.name} (part {p} of {nparts}): {E.first_mismatch(gi.mem.get(gi.view), wi)}")
            done = rows[p + 1] * k
            below, above = go.view[:done], go.view[done:]
            if not go.mem.eq(below, go.mem.const(full[:done])):
                self.wrong(go, go.mem.get(go.view)[:done], full[:done], f"after part {p} of {nparts}, side {side} k {k}, rows below "
                           f"{rows[p + 1]} are not final; cuts {rows}", kind="rows below the cut")
            if not go.mem.all_bits(above, go.prefill):
                self.fail("rows above the cut", f"after part {p} of {nparts} on {H.name} side {side} k {k} rows from {rows[p + 1]} on were "
                          f"written (cuts {rows})")
            if p + 1 < nparts:
                self.between_parts(H)
        if rc == FS_OK:
            rc2, again = self.call(H.A.part_rows, nparts, bool(side), k)
            if rc2 != FS_OK or again != rows:
                self.fail("part rows", f"cuts of {H.name} side {side} nparts {nparts} moved: {rows} before the product, {again} after")
            if k > 1:
                self.counts["k"][side].add(k)
        self.check_all(H, [(gi, wi, "x")], [(go, full, f"in {nparts} parts, side {side} k {k}")] if rc == FS_OK else [])
        return rc

    def op_prepare(self, H, k=None, side=None):
        k = int(self.rng.choice(self.ks)) if k is None else k
        side = int(self.rng.integers(2)) if side is None else side
        m = H.model
        if side and not m.has_t:
            want = FS_ERR_NO_TRANSPOSE
        else:
            # what prepare still has to do reads the plain arrays: building the k-column two-pass copy (bit 0), timing column sweeps
            # against the row kernel (bit 1); allocating scratch (bit 2) does not
            want = FS_ERR_RELEASED if m.released[side] and (self.b.spmm_needs(H.A, k, side, self.b.creation_options(H.copy)) & 3) else FS_OK
        self.note(f"{H.name} prepare k {k} side {side}")
        with self.b.options(**self.b.creation_options(H.copy)):       # one-time work, like creation: under the options of creation
            rc, _ = self.call(H.A.prepare, k, self.b.stream(), transposed=bool(side))
        self.expect(H, f"fs_matrix_prepare({k})", rc, want)
        if rc != FS_ERR_NO_TRANSPOSE:
            m.prepared[side].add(k)         # (a prepare refused half way may have made part of what it makes: the scratch)
        self.check_all(H)
        return rc

    def op_release_prepared(self, H, k=None):
        if k is None:
            k = 0 if self.rng.integers(3) == 0 else int(self.rng.choice(self.ks))
        self.note(f"{H.name} release_prepared {k}")
        rc, n = self.call(H.A.release_prepared, k)
        self.expect(H, "fs_matrix_release_prepared", rc, FS_OK)
        m = H.model
        for side in (0, 1) if m.has_t else (0,):
            # k = 2 and 3 share the two-column two-pass copy; the column-major scratch of an LDS-staged copy goes k by k
            gone = set(self.ks) if k == 0 else {2, 3} if k in (2, 3) and m.kept[side] != 8 else {k}
            m.prepared[side] -= gone
            for kk in sorted(gone):
                plan = self.b.spmm_plan(H.A, kk, side)
                if plan == KCOL_PLAN or (k == 0 and plan == LDSX_COLUMNS_PLAN):
                    self.fail("release_prepared", f"after release_prepared({k}) on {H.name} fs_matrix_spmm_plan({kk}, side {side}) is still "
                              f"{plan}: a plan that needs what prepare made")
        if (k == 0 or not (m.prepared[0] | m.prepared[1])) and H.A.device_bytes()[2] != 0:
            self.fail("device bytes", f"after release_prepared({k}) nothing prepared is left on {H.name} and it still reports "
                      f"{H.A.device_bytes()} ([2] must be 0)")
        self.check_all(H)

    def op_prepare_roundtrip(self, H):
        """prepare(k) then release_prepared(k) on a handle that holds nothing prepared: fs_matrix_device_bytes is back where it was"""
        self.op_release_prepared(H, 0)
        before = H.A.device_bytes()
        k, side = int(self.rng.choice([k for k in self.ks if k <= 16])), int(self.rng.integers(2)) if H.model.has_t else 0
        self.op_prepare(H, k, side)
        self.op_release_prepared(H, k)
        after = H.A.device_bytes()
        if after != before:
            self.fail("device bytes", f"prepare({k}) then release_prepared({k}) on {H.name}: {before} before, {after} after")

    def op_release_csr(self, H):
        m = H.model
        want = m.release_csr()
        self.note(f"{H.name} release_csr")
        rc, n = self.call(H.A.release_csr)
        self.expect(H, "fs_matrix_release_csr", rc, FS_OK)
        if n != want:
            self.fail("bookkeeping", f"fs_matrix_release_csr({H.name}) released {n} side(s), the model says {want} (kept {m.kept}, released {m.released})")
        b = H.A.device_bytes()
        if m.all_released() and b[0] != 0:
            self.fail("device bytes", f"every side of {H.name} is released and it still reports {b} ([0] must be 0)")
        self.check_all(H)

    def op_restore_csr(self, H):
        m = H.model
        side = int(self.rng.integers(2))
        released = [s for s in (0, 1) if m.released[s]]
        if released and self.rng.integers(4):
            side = released[int(self.rng.integers(len(released)))]
        borrow = bool(self.rng.integers(2))
        self.note(f"{H.name} restore_csr side {side} {'borrowed' if borrow else 'copied'}")
        if borrow and m.released[side] and (not side or m.has_t):
            for which in ("row_ptr", "cols", "vals"):            # the arrays handed over before are the caller's again
                H.arrays.pop((side, which), None)
                H.array_consts.pop((side, which), None)
            rp, cc, vv = self.arrays_for(H, side)
        else:
            rp, cc, vv = (self.b.mem.const(a) if a is not None else None for a in H.refs.csr[side])
        want = FS_ERR_ARG if side and not m.has_t else FS_OK
        rc, _ = self.call(H.A.restore_csr, rp, cc, vv, transposed=bool(side), borrow=borrow)
        self.expect(H, "fs_matrix_restore_csr", rc, want)
        if rc == FS_OK:
            if m.released[side]:
                self.counts["restore"].add("borrowed" if borrow else "copied")
            m.released[side] = False
        self.check_all(H)

    def op_download(self, H):
        m = H.model
        side = int(self.rng.integers(2))
        want = FS_ERR_NO_TRANSPOSE if side and not m.has_t else FS_ERR_RELEASED if m.released[side] else FS_OK
        self.note(f"{H.name} download side {side}")
        rc, got = self.call(H.A.download, bool(side))
        self.expect(H, "fs_matrix_download", rc, want)
        if rc == FS_OK:
            for name, g, w in zip(("row_ptr", "cols", "vals"), got, H.refs.csr[side]):
                if w is not None and not np.array_equal(np.asarray(g).view(np.int64 if w.dtype == np.float64 else w.dtype), w.view(np.int64 if w.dtype == np.float64 else w.dtype)):
                    self.fail("download", f"{name} of side {side} of {H.name} differs from the array that went in")
        self.check_all(H)

    def op_flip(self, H):
        changed = [n for n, vals in FLIPS.items() if self.o[n] != self.neutral[n]]
        if changed and self.rng.integers(2):
            name = changed[int(self.rng.integers(len(changed)))]
            value = self.neutral[name]
        else:
            name = list(FLIPS)[int(self.rng.integers(len(FLIPS)))]
            value = FLIPS[name][int(self.rng.integers(len(FLIPS[name])))]
            if value == "own":
                value = H.model.kept[0] if H.model.kept[0] >= 6 else 0
        self.flip(name, value)

    def op_stream(self, H):
        self.b.switch_stream()
        self.note(f"stream {self.b.stream_index()}")

    def op_churn(self, H):
        if H.pair is not None:              # a pair goes and comes as a whole; the exact one comes back as its twin
            pair = H.pair
            self.note(f"destroy the pair {pair.A.name}, {pair.At.name}")
            self.destroy(pair.A)
            self.destroy(pair.At)
            self.pairs.remove(pair)
            self.check_all(None)
            self.create_pair(pair.ps.kind, valued=not pair.ps.fam.valued if pair.ps.fam else False)
            return
        self.note(f"destroy {H.name}")
        self.destroy(H)
        self.check_all(None)
        self.create()

    def op_build_transpose(self, H):
        m = H.model
        want = FS_OK if m.has_t or not m.released[0] else FS_ERR_RELEASED
        self.note(f"{H.name} build_transpose")
        with self.b.options(**self.neutral), self.b.options(**self.b.creation_options(H.copy)):
            rc, _ = self.call(H.A.build_transpose, self.b.stream())
            self.expect(H, "fs_matrix_build_transpose", rc, want)
            if rc == FS_OK and not m.has_t:
                m.has_t = True
                self.learn_side(H, 1)
                H.base_bytes = H.A.device_bytes()
        self.check_all(H)

    def op_bad_arg(self, H):
        which = int(self.rng.integers(3))
        gi, wi = self.place_in(H, "in", 0, 0, 1)
        go = self.place_out(H, "out", 0, 1)
        self.note(f"{H.name} bad argument {('spmm k = 0', 'spmv_part part = nparts', 'prepare k = 0')[which]}")
        if which == 0:
            rc, _ = self.call(H.A.spmm, go.view, gi.view, 0, self.b.stream())
        elif which == 1:
            rc, _ = self.call(H.A.spmv_part, go.view, gi.view, 3, 3, self.b.stream())
        else:
            rc, _ = self.call(H.A.prepare, 0, self.b.stream())
        self.expect(H, "a call with a bad argument", rc, FS_ERR_ARG)
        self.check_all(H, [(gi, wi, "x")])
        if not go.mem.all_bits(go.view, go.prefill):
            self.fail("not exact", f"a refused call wrote into {go.name}")

    # -- solver pairs ----
    def create_pair(self, kind, valued=False):
        ps = pair_system(kind, valued)
        HA, HT = self.create(data=ps.data[0]), self.create(data=ps.data[1])
        pair = Pair(ps, HA, HT)
        HA.pair = HT.pair = pair
        F = ps.s.ncol
        for role, cap in (("x", max(N.MAX_RHS * F, S.MAX_SHIFTS * (F + 3), 8 * (max(MSCGN_KS) * F + 3))), ("b", N.MAX_RHS * F), ("diag", F), ("d", F)):
            HA.vec["solve " + role] = Guarded(self.b.mem, f"{role} of the solvers on {HA.name}", cap)
        self.pairs.append(pair)
        return pair

    def pair_state(self, pair):
        return ({n: self.b.get_option(n) for n in FLIPS}, [self.b.kernel_code(h.A, 0) for h in (pair.A, pair.At)],
                [h.A.device_bytes() for h in (pair.A, pair.At)])

    def poison(self, pair, sizes):
        seen, probed = self.b.poison_heap(sizes)
        self.counts["poison_seen"] += seen
        self.counts["poison_probed"] += probed
        self.counts["poisoned"] += 1
        self.log.append(f"{self.step:4d} poison_heap({sorted(set(sizes))}): the probe saw {seen} of {probed}")

    def products_status(self, pair, k, jacobi=False):
        """what the header promises for a solve whose products take k columns, from the state of the two handles: FS_ERR_RELEASED for
        Jacobi on a released At, from fs_matrix_prepare for a k that still needs the plain arrays of a released side, and from
        the products themselves.  For k >= 2 the last is known once the solver's own prepare has settled the plan: None then"""
        if jacobi and pair.At.model.released[0]:
            return FS_ERR_RELEASED
        if k == 1:
            return FS_ERR_RELEASED if any(h.model.product(0, self.o) != FS_OK for h in (pair.A, pair.At)) else FS_OK
        for h in (pair.A, pair.At):
            if h.model.prepare_refused(0, self.b.spmm_needs(h.A, k, 0, {})):
                h.model.prepared[0].add(k)                  # (refused half way: see op_prepare)
                return FS_ERR_RELEASED
            h.model.prepared[0].add(k)
        return None

    def usable_widths(self, pair, k, needs):
        """after a solve under option "pcgn_compact" that answered FS_OK: the rungs below k it may have narrowed to, from the Models of
        the two handles (a refused width is silent).  needs: {w: fs_debug_spmm_needs of both handles before the solve}.  The solve
        ran fs_matrix_prepare for every rung from 2 on, on A and, where A's went through, on At"""
        usable = []
        for w in sorted(needs, reverse=True):
            hs = (pair.A, pair.At)
            if w >= 2:
                pair.A.model.prepared[0].add(w)
                if not pair.A.model.prepare_refused(0, needs[w][0]):
                    pair.At.model.prepared[0].add(w)
            plans = [self.b.spmm_plan(h.A, w, 0) if w >= 2 else None for h in hs]
            if all(h.model.width_usable(0, w, nd, pl, self.o) for h, nd, pl in zip(hs, needs[w], plans)):
                usable.append(w)
        return usable

    def run_solver(self, pair, solver, what, kw, want_x=None, x0=None, ldx=None, off8=None, k=1, jacobi=False, want=None, poison=None,
                   null=(), raw=None):
        """one solver call on the pair inside the frame of checks.  kw: the arguments of solve_model (b, lam, tol, max_iter, precond,
        x0, diag, lams); want: the status, or None for what products_status says; raw: arguments of backend.solve that replace
        the ones derived from kw (the bad arguments).  Returns (status, Solved or None)."""
        b_, mem, s = self.b, self.b.mem, pair.ps.s
        F, hA = s.ncol, pair.A
        m = len(kw["lams"]) if solver in LADDERS else 1
        ne = F * k if solver == "mscgn" else F                 # one vector / panel of X
        ldx = ne if ldx is None else ldx
        off8 = int(self.rng.integers(2)) if off8 is None else off8
        nx = (m - 1) * ldx + ne if solver in LADDERS else F * (2 if solver == "cg2" else k)
        gx, gb, gd = hA.vec["solve x"], hA.vec["solve b"], hA.vec["solve diag"]
        before_x = np.full(nx, PREFILLS["nan"], np.int64).view(np.float64)
        if x0 is not None:
            before_x = np.array(x0, np.float64).reshape(-1)
        mem.put(gx.place(nx, off8), before_x)
        b = np.ascontiguousarray(kw["b"], np.float64).reshape(-1)
        mem.put(gb.place(b.size, off8 if solver in K_COLUMNS + ("cg2",) else int(self.rng.integers(2))), b)
        ins = [(gb, b, "b")]
        diag = kw.get("diag")
        if diag is not None:
            mem.put(gd.place(F, int(self.rng.integers(2))), diag)
            ins.append((gd, diag, "diag"))
        args = dict(lam=kw.get("lam", s.lam), tol=kw.get("tol", s.tol), max_iter=kw.get("max_iter", 0), precond=kw.get("precond", P.PRECOND_NONE),
                    warm=x0 is not None, diag=None if diag is None else gd.view, k=m if solver == "mscg" else k, lams=kw.get("lams", ()), ldx=ldx, null=null,
                    m=m)
        args.update(raw or {})
        if want is None:
            want = self.products_status(pair, 2 if solver == "cg2" else k, jacobi)
        kk = 2 if solver == "cg2" else k                    # the columns of the solve's products
        needs = [self.b.spmm_needs(h.A, kk, 0, {}) if kk >= 2 else 0 for h in (pair.A, pair.At)]
        narrows = solver in NARROWING and self.o["pcgn_compact"] == 1
        rungs = [w for w in PM.RUNGS if w < k] if narrows else []
        wneeds = {w: [self.b.spmm_needs(h.A, w, 0, {}) if w >= 2 else 0 for h in (pair.A, pair.At)] for w in rungs}
        before = self.pair_state(pair)
        if poison if poison is not None else bool(self.rng.integers(2)):
            nslots = len([v for v in kw["lams"] if v != min(kw["lams"])]) if solver in LADDERS else 0
            sizes = work_space(solver, F, s.nrow, 2 if solver == "cg2" else k, args["precond"] != P.PRECOND_NONE, nslots,
                               widths=(rungs[-1], rungs[-2] if len(rungs) > 1 else 0) if rungs else ())
            # (which rungs are usable is known behind the solve: the panels of every rung it could settle on, besides the widest two)
            self.poison(pair, sizes + [w * F for w in rungs])
        self.note(f"{what} on {hA.name} / {pair.At.name}, x {nx} doubles 8 * {off8} off, ldx {ldx}")
        self.counts["solves"][solver] = self.counts["solves"].get(solver, 0) + 1
        rc, res = self.call(b_.solve, solver, pair.A.A, pair.At.A, gx.view, gb.view, **args)
        if want is None:                                    # the solver's prepare went through: the plans say what the products need
            plans = [b_.spmm_plan(h.A, kk, 0) for h in (pair.A, pair.At)]
            want = FS_ERR_RELEASED if any(h.model.multi(0, pl) != FS_OK for h, pl in zip((pair.A, pair.At), plans)) else FS_OK
        self.expect(hA, what, rc, want)
        self.counts["solver_status"][(solver, want)] = self.counts["solver_status"].get((solver, want), 0) + 1
        self.check_all(hA, ins)
        got = mem.get(gx.view)
        model = None
        if rc != FS_OK:
            if not E.bits_equal(got, before_x):
                self.fail("x written", f"{what} returned {STATUS_NAMES.get(rc, rc)} and wrote to x all the same: {E.first_mismatch(got, before_x)}")
        else:
            model = solve_model(pair.ps, solver, b, args["lam"], args["tol"], args["max_iter"], args["precond"], x0, diag, kw.get("lams"))
            full = before_x.copy()
            if solver in LADDERS:
                gaps = np.ones(nx, bool)
                for i in range(m):
                    full[i * ldx:i * ldx + ne] = np.ascontiguousarray(model.x[i]).reshape(-1)
                    gaps[i * ldx:i * ldx + ne] = False
                if not np.array_equal(got.view(np.int64)[gaps], before_x.view(np.int64)[gaps]):
                    self.fail("gap written", f"{what}: a gap between the vectors of X (ldx {ldx}, {ne} doubles each) was written, first at "
                              f"{int(np.flatnonzero(gaps & (got.view(np.int64) != before_x.view(np.int64)))[0])}")
            else:
                full = np.ascontiguousarray(model.x).reshape(-1)
            if not E.bits_equal(got, full):
                self.wrong(gx, got, full, what)
            if res["iters"] != model.iters:
                self.fail("not exact", f"{what}: iterations {res['iters']}, the model {model.iters}")
            for j, (g, w) in enumerate(zip(res["infos"] or [], model.infos or [])):
                if (g[0], g[1]) != (w.iterations, w.converged) or not (M.same_bits(g[2], w.rnorm)[0] and M.same_bits(g[3], w.bnorm)[0]):
                    self.fail("not exact", f"{what}: fs_pcg_info[{j}] = {g}, the model {tuple(w)}")
            if solver in NARROWING:
                self.check_segments(pair, what, k, self.usable_widths(pair, k, wneeds), model, args["max_iter"] or F)
        after = self.pair_state(pair)
        if after[0] != before[0]:
            self.fail("option", f"{what} changed options: {[(n, before[0][n], after[0][n]) for n in FLIPS if before[0][n] != after[0][n]]}")
        if after[1] != before[1]:
            self.fail("bookkeeping", f"fs_matrix_spmv_kernel of the pair was {before[1]} before {what} and is {after[1]} after it (a scope "
                      "that was not given back?)")
        for i, (h, b0, b1, nd) in enumerate(zip((pair.A, pair.At), before[2], after[2], needs)):
            grew = rc == FS_OK and kk >= 2 and (nd & 5)
            may_grow = (kk >= 2 and (nd & 5)) or (rc == FS_OK and any(wneeds[w][i] & 5 for w in wneeds))    # (the rungs' one-time work)
            if b1[2] < b0[2] or (b1[2] != b0[2] and not may_grow) or b1[1] < b0[1] or b1[1] > h.base_bytes[1] + self.b.lazy_growth(h.A):
                self.fail("device bytes", f"{h.name} reported {b0} before {what} and {b1} after it (prepare needs {nd}, after creation {h.base_bytes})")
            if grew and (self.b.spmm_needs(h.A, kk, 0, {}) & 5):
                self.fail("bookkeeping", f"after {what} fs_matrix_prepare({kk}) still has work on {h.name}: the solve did not do its one-time work")
        pair.A.prove = pair.At.prove = True                 # the next product on either handle: exact
        return rc, model

    def check_segments(self, pair, what, k, usable, model, cap):
        """fs_debug_last_pcgn_segments of the solve just made against tests/_pcgn_plan_model.py on the model's counts: one segment of
        all k columns without option "pcgn_compact"; with it the schedule on the usable widths.  A column is frozen by the start
        kernels where its model never took r.z"""
        segs = self.b.last_segments()
        want = PM.plan(k, usable, model.iters, ["rsq" not in st for st in model.extra], cap)
        self.log[-1] += f", usable widths {usable}, segments {segs}"
        if segs != want:
            self.fail("segments", f"{what}: fs_debug_last_pcgn_segments says {segs}, the plan model on the usable widths {usable} and "
                      f"the counts {model.iters} says {want} (options {self.o})")
        if any(w < k for _, w, _ in segs):
            self.counts["repacked"] += 1

    def op_gram_diag(self, H):
        pair = H.pair
        lam = float((0.0, 0.75, pair.ps.s.lam)[int(self.rng.integers(3))])
        gd = pair.A.vec["solve d"]
        F = pair.ps.s.ncol
        self.b.mem.fill_bits(gd.place(F, int(self.rng.integers(2))), PREFILLS["nan"])
        want = FS_ERR_RELEASED if pair.At.model.released[0] else FS_OK
        before = self.pair_state(pair)
        self.note(f"fs_gram_diag({pair.At.name}, {lam})")
        rc, _ = self.call(self.b.gram_diag, pair.At.A, lam, gd.view)
        self.expect(pair.At, "fs_gram_diag", rc, want)
        self.counts["solver_status"][("gram_diag", want)] = self.counts["solver_status"].get(("gram_diag", want), 0) + 1
        self.check_all(pair.A)
        got = self.b.mem.get(gd.view)
        if rc == FS_OK:
            d = P.gram_diag(pair.ps.t_csr, lam)
            if not E.bits_equal(got, d):
                self.wrong(gd, got, d, f"fs_gram_diag lambda {lam}")
            if lam == pair.ps.s.lam:
                pair.saved_diag = d                         # the caller's diagonal of later FS_PRECOND_DIAG solves
        elif not (got.view(np.int64) == PREFILLS["nan"]).all():
            self.fail("x written", "the refused fs_gram_diag wrote to d")
        if self.pair_state(pair) != before:
            self.fail("bookkeeping", f"fs_gram_diag changed options, kernels or device bytes: {before} -> {self.pair_state(pair)}")

    def exact_solve(self, H, solver, poison=None, pick=None):
        pair = H.pair
        fam = pair.ps.fam
        cases = [c for c in exact_cases(fam) if c[0] == solver]
        if pick is None and solver in NARROWING and self.o["pcgn_compact"] == 1 and self.rng.integers(2):
            # half of the solves of a walk that narrows: panels of 3, 5 and 17 columns, which freeze columns at the start and so repack
            cases = [c for c in cases if c[2]["b"].size // fam.F in (3, 5, 17)]
        _, what, kw = cases[int(self.rng.integers(len(cases))) if pick is None else pick % len(cases)]
        kw = dict(kw, lam=fam.s.lam, tol=fam.s.tol)
        if kw.get("precond") == P.PRECOND_DIAG and pair.saved_diag is not None and self.rng.integers(2):
            kw["diag"], what = pair.saved_diag, what + " (the diagonal of an earlier fs_gram_diag)"
        k = kw["b"].size // fam.F if solver in K_COLUMNS else 1
        ldx = fam.F * k + 3 * int(self.rng.integers(2)) if solver in LADDERS else None
        return self.run_solver(pair, solver, what, kw, x0=kw.get("x0"), ldx=ldx, k=k, jacobi=kw.get("precond") == P.PRECOND_JACOBI, poison=poison)

    def op_cg(self, H):
        self.exact_solve(H, "cg")

    def op_cg2(self, H):
        self.exact_solve(H, "cg2")

    def op_pcg(self, H):
        self.exact_solve(H, "pcg")

    def op_mscg(self, H):
        self.exact_solve(H, "mscg")

    def op_pcgn(self, H):
        self.exact_solve(H, "pcgn")

    def op_pcgn_lambdas(self, H):
        self.exact_solve(H, "pcgn_lambdas")

    def op_mscgn(self, H):
        self.exact_solve(H, "mscgn")

    def op_solve_strict(self, H, pick=None, poison=None):
        """strict_order on through the walk's own flip (the Model knows), one solver on the general system against its model, x,
        counts, info and the state of the debug hooks bit for bit; then the option as it was"""
        pair = H.pair
        saved = self.o["strict_order"]
        self.flip("strict_order", 1)
        try:
            cases = strict_cases(pair.ps)
            solver, what, kw = cases[int(self.rng.integers(len(cases))) if pick is None else pick % len(cases)]
            k = kw["b"].size // pair.ps.s.ncol if solver in K_COLUMNS else 1
            ldx = pair.ps.s.ncol * k + 3 * int(self.rng.integers(2)) if solver == "mscgn" else None
            rc, model = self.run_solver(pair, solver, what + " under strict_order", kw, x0=kw.get("x0"), k=k, ldx=ldx,
                                        jacobi=kw.get("precond") == P.PRECOND_JACOBI, poison=poison)
            if rc == FS_OK:
                bad = self.state_mismatch(solver, model, len(kw.get("lams", ())), k)
                if bad:
                    self.fail("not exact", f"{what} under strict_order, the state of the debug hooks: {bad}")
        finally:
            self.flip("strict_order", saved)
        return rc

    def state_mismatch(self, solver, model, m, k):
        st = self.b.last_state(solver, m if solver == "mscg" else k, m)
        if st is None:
            return None
        state, extra = st
        bad = M.mismatch(np.zeros(0), np.zeros(0), None, None, state, model.state if solver not in K_COLUMNS else None)
        if bad or solver in ("cg", "pcg"):
            return bad
        if solver == "mscgn":                               # fs_debug_last_mscgn_state(j): every column against its fs_mscg model
            for j, (want_st, want_sh) in enumerate(model.extra):
                bad = M.mismatch(np.zeros(0), np.zeros(0), None, None, extra[j][0], want_st) or S.shifts_mismatch(extra[j][1], want_sh)
                if bad:
                    return f"column {j}: {bad}"
            return None
        if solver == "mscg":
            return S.shifts_mismatch(extra, model.extra)
        for j, want in enumerate(model.extra):              # fs_pcgn, fs_pcgn_lambdas: the scalars of every column against its fs_pcg model
            for key, name in (("rr", "rr"), ("bb", "bb"), ("stop", "stop"), ("rsq", "rz"), ("alpha", "alpha"), ("beta", "beta")):
                if key in want and not M.same_bits(extra[j][name], want[key])[0]:
                    return f"column {j} {name}: got {float(extra[j][name])!r} want {float(want[key])!r}"
            if extra[j]["count"] != want["iter"] or extra[j]["converged"] != want["done"]:
                return f"column {j}: count {extra[j]['count']} converged {extra[j]['converged']}, the model {want['iter']} {want['done']}"
        return None

    BAD_ARGS = [("pcg", "NULL A", dict(null=("A",))), ("mscg", "NULL At", dict(null=("At",))), ("pcgn", "NULL x", dict(null=("x",))),
                ("cg", "NULL b", dict(null=("b",))), ("pcg", "NULL prm", dict(null=("prm",))), ("pcgn", "NULL prm", dict(null=("prm",))),
                ("mscg", "NULL lambda", dict(null=("lambda",))), ("cg2", "NULL x", dict(null=("x",))),
                ("cg", "A twice", dict(twice=True)), ("pcg", "A twice", dict(twice=True)), ("mscg", "A twice", dict(twice=True)),
                ("pcgn", "A twice", dict(twice=True)), ("cg2", "A twice", dict(twice=True)),
                ("pcgn", "k = 0", dict(k=0)), ("pcgn", "k = 33", dict(k=33)), ("mscg", "m = 0", dict(k=0)), ("mscg", "m = 17", dict(k=17)),
                ("mscg", "ldx < F", dict(ldx=-1)), ("pcg", "tol < 0", dict(tol=-1e-8)), ("pcgn", "tol NaN", dict(tol=float("nan"))),
                ("mscg", "tol NaN", dict(tol=float("nan"))), ("mscg", "tol < 0", dict(tol=-1.0)),
                ("mscg", "lambda NaN", dict(lams=[1.0, float("nan"), 5.0])), ("mscg", "lambda inf", dict(lams=[float("inf"), 1.0, 5.0])),
                ("pcg", "precond = 3", dict(precond=3)), ("pcgn", "precond = 3", dict(precond=3)),
                ("pcg", "DIAG with NULL diag", dict(precond=P.PRECOND_DIAG)), ("pcgn", "DIAG with NULL diag", dict(precond=P.PRECOND_DIAG)),
                # fs_pcgn_lambdas and fs_mscgn
                ("pcgn_lambdas", "NULL A", dict(null=("A",))), ("mscgn", "NULL A", dict(null=("A",))),
                ("pcgn_lambdas", "NULL At", dict(null=("At",))), ("mscgn", "NULL At", dict(null=("At",))),
                ("pcgn_lambdas", "NULL x", dict(null=("x",))), ("mscgn", "NULL x", dict(null=("x",))),
                ("pcgn_lambdas", "NULL b", dict(null=("b",))), ("mscgn", "NULL b", dict(null=("b",))),
                ("pcgn_lambdas", "NULL lambda", dict(null=("lambda",))), ("mscgn", "NULL lambda", dict(null=("lambda",))),
                ("pcgn_lambdas", "NULL prm", dict(null=("prm",))), ("pcgn_lambdas", "A twice", dict(twice=True)), ("mscgn", "A twice", dict(twice=True)),
                ("pcgn_lambdas", "k = 0", dict(k=0)), ("pcgn_lambdas", "k = 33", dict(k=33)), ("mscgn", "k = 0", dict(k=0)), ("mscgn", "k = 33", dict(k=33)),
                ("mscgn", "m = 0", dict(m=0)), ("mscgn", "m = 17", dict(m=17)), ("mscgn", "ldx < F k", dict(ldx=-1)),
                ("pcgn_lambdas", "lambda NaN", dict(lams=[1.0, float("nan"), 5.0])), ("pcgn_lambdas", "lambda inf", dict(lams=[float("inf"), 1.0, 5.0])),
                ("mscgn", "lambda NaN", dict(lams=[1.0, float("nan"), 5.0])), ("mscgn", "lambda -inf", dict(lams=[1.0, 5.0, float("-inf")])),
                ("pcgn_lambdas", "tol < 0", dict(tol=-1e-8)), ("pcgn_lambdas", "tol NaN", dict(tol=float("nan"))),
                ("mscgn", "tol < 0", dict(tol=-1.0)), ("mscgn", "tol NaN", dict(tol=float("nan"))),
                ("pcgn_lambdas", "precond = 3", dict(precond=3)), ("pcgn_lambdas", "DIAG with NULL diag", dict(precond=P.PRECOND_DIAG))]

    def op_solve_bad_arg(self, H, pick=None):
        pair = H.pair
        s = pair.ps.s
        solver, what, raw = self.BAD_ARGS[int(self.rng.integers(len(self.BAD_ARGS))) if pick is None else pick % len(self.BAD_ARGS)]
        raw = dict(raw)
        k = 3 if solver in K_COLUMNS else 1
        i = np.arange(s.ncol * max(k, 2), dtype=np.float64)
        kw = dict(b=(i % 7 - 3.0)[:s.ncol * (2 if solver == "cg2" else k)], lam=s.lam, tol=1e-6, max_iter=2)
        if solver in LADDERS + ("pcgn_lambdas",):
            kw["lams"] = [s.lam + 4.0, s.lam, s.lam + 12.0]
            if solver == "mscg" and ("k" in raw or "lams" in raw) or solver == "mscgn" and "m" in raw:
                raw.setdefault("lams", [s.lam] * 17)
            if raw.get("ldx") == -1:
                raw["ldx"] = s.ncol * k - 1
        twice = raw.pop("twice", False)
        if twice:
            pair = Pair(pair.ps, pair.A, pair.A)            # At not of the transposed shape
        try:
            self.run_solver(pair, solver, f"fs_{solver} with {what}", kw, k=k, want=FS_ERR_ARG, raw=raw, null=raw.pop("null", ()))
        finally:
            H.pair.At.prove = True


    def recover(self, H):
        """the very next product on a handle that has just refused a call: exact.  Under the options of the moment where the model
        says they allow one, else with strict_order / spmv_kernel / reproducible at their defaults for this one product."""
        H.prove = False
        self.counts["recovered"] += 1
        if H.model.product(0, self.o) == FS_OK:
            rc = self.op_spmv(H, 0)
        else:
            keys = ("strict_order", "spmv_kernel", "reproducible")
            saved = {k: self.o[k] for k in keys}
            with self.b.options(**{k: self.neutral[k] for k in keys}):
                self.o.update({k: self.neutral[k] for k in keys})
                try:
                    rc = self.op_spmv(H, 0)
                finally:
                    self.o.update(saved)
        H.prove = False
        if rc != FS_OK:
            self.fail("status", f"the product behind a refused call on {H.name} was refused too")

    def end_of_life(self, H):
        """no growth over the walk: with nothing prepared the handle holds what it held after creation (and the two-byte row ids a
        one-byte two-pass copy may have made on its first fixed-order product)"""
        self.op_release_prepared(H, 0)
        b, base = H.A.device_bytes(), H.base_bytes
        if b[2] != 0 or b[1] < base[1] or b[1] > base[1] + self.b.lazy_growth(H.A):
            self.fail("device bytes", f"{H.name} held {base} after creation and {b} at the end of the walk")

    # -- the loop ----
    def choose(self, H):
        m = H.model
        names = list(OPS)
        w = np.array([OPS[n] for n in names], float)
        for i, n in enumerate(names):
            if n == "ata" and not H.refs.ata:
                w[i] = 0
            if n == "build_transpose" and m.has_t:
                w[i] = 0.5
            if n == "churn" and (self.step < 10 or H is self.handles[0]):      # the copy the walk is named for stays to the end
                w[i] = 0
            if n in SOLVER_OPS:
                kind = None if H.pair is None else H.pair.ps.kind
                if kind is None or (kind == "exact" and n == "solve_strict") or (kind == "general" and n in EXACT_ONLY):
                    w[i] = 0
        return names[int(self.rng.choice(len(names), p=w / w.sum()))]

    @contextlib.contextmanager
    def session(self):
        """the frame of a walk, also for tests that drive the operations by hand: whatever is flipped inside is put back on the way
        out, the handles made inside are destroyed"""
        b = self.b
        self.neutral = {n: b.get_option(n) for n in FLIPS}
        self.o = dict(self.neutral)
        with b.options(**self.neutral), b.walk_scope():
            try:
                self.step = -1
                yield self
            finally:
                for h in list(self.handles):
                    h.A.close()
                self.handles, self.pairs = [], []

    def flip(self, name, value):
        self.note(f"option {name} = {value}")
        self.b.set_option(name, value)
        self.o[name] = value

    def run(self):
        b = self.b
        with self.session():
            if True:
                self.create(first=True)
                for _ in range(self.nhandles - 1):
                    self.create()
                if self.solvers:
                    self.create_pair("exact", valued=bool(self.rng.integers(2)))
                    self.create_pair("general")
                for self.step in range(self.steps):
                    b.begin_step(self.step)
                    H = self.handles[int(self.rng.integers(len(self.handles) + 1)) % len(self.handles)]    # (the first one twice as often)
                    op = self.choose(H)
                    self.count(op)
                    if op in ("spmv", "spmv_t"):
                        self.op_spmv(H, int(op == "spmv_t"))
                    elif op in ("spmv_host", "spmv_t_host"):
                        self.op_spmv(H, int(op == "spmv_t_host"), host=True)
                    elif op in ("spmm", "spmm_t"):
                        self.op_spmm(H, int(op == "spmm_t"))
                    elif op == "spmv_part":
                        self.op_part(H, int(self.rng.integers(4) == 0), 1)
                    elif op == "spmm_part":
                        self.op_part(H, int(self.rng.integers(2)), int(self.rng.choice([k for k in (2, 4) if k <= self.kmax])))
                    else:
                        getattr(self, "op_" + op)(H)
                    for h in self.handles:
                        self.bookkeeping(h)
                        if h.prove:
                            self.recover(h)
                if self.steps:
                    self.step = self.steps
                    b.begin_step(self.step)
                    for h in self.handles:
                        self.end_of_life(h)
        return self


def run_walk(backend, data, copy, seed, steps=150, upto=None, **kw):
    """one walk; raises WalkFailure at the first failing check.  upto=N: only the first N steps of the same walk."""
    return Walk(backend, data, copy, seed, steps=steps, upto=upto, **kw).run()


# ---- the real library ----------------------------------------------------------------------------------------------------
class HipBackend:
    """libfastsparse_hip.so through libfastsparse_amd.capi; vectors in HBM through torch; two streams (torch's default stream and
    one of the walk's own), products and checks on torch's current stream"""
    def __init__(self, paths, options):
        import ctypes as C
        import torch
        from libfastsparse_amd import capi
        self.C, self.torch, self.capi = C, torch, capi
        self.paths, self.options = paths, options
        self.Error = capi.FastsparseError
        self.mem, self.hostmem = TorchMem(), NumpyMem()
        self.L = L = capi.lib()
        L.fs_debug_ldsx_orderable.argtypes = [C.c_void_p, C.c_int]
        L.fs_debug_tiled_layout.argtypes = [C.c_void_p, C.c_int]
        L.fs_debug_spmm_needs.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.fs_debug_two_pass_rows8.restype = C.c_longlong
        L.fs_debug_two_pass_rows8.argtypes = [C.c_void_p, C.c_int]
        L.fs_debug_two_pass_layout.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]
        L.fs_debug_last_spmm_plan.argtypes = []
        self.streams = [torch.cuda.default_stream(), torch.cuda.Stream()]
        self.cur = 0

    def copies(self):
        return list(self.paths) + [AUTO]

    def creation_options(self, copy):
        return {} if copy == AUTO else dict(self.paths[copy][0])

    def get_option(self, name):
        v = self.L.fs_get_option(name.encode())
        assert v != FS_ERR_ARG, name
        return v

    def set_option(self, name, value):
        self.capi.set_option(name, value)

    @contextlib.contextmanager
    def walk_scope(self):
        self.cur = 0
        try:
            with self.torch.cuda.stream(self.streams[0]):
                yield
        finally:
            self.torch.cuda.synchronize()
            self.torch.cuda.set_stream(self.streams[0])

    def begin_step(self, i):
        pass

    def stream(self):
        return self.streams[self.cur].cuda_stream

    def stream_index(self):
        return self.cur

    def switch_stream(self):
        """products on one handle must not overlap: the new stream waits for the old one (an event), the host does not"""
        ev = self.torch.cuda.Event()
        ev.record(self.streams[self.cur])
        self.cur ^= 1
        self.streams[self.cur].wait_event(ev)
        self.torch.cuda.set_stream(self.streams[self.cur])

    def create(self, d, copy, arrays, borrow, must=True):
        rp, cc, vv = arrays
        if not borrow:
            rp, cc, vv = (None if a is None else self.mem.const(a) for a in arrays)
        A = self.capi.Matrix.from_csr(d.nrow, d.ncol, rp, cc, vv, borrow=borrow)
        if copy != AUTO and must:
            want = {"stream": 1, "two-pass": 7, "lds-staged": 8, "tiled": 6}[self.paths[copy][1]]
            assert self.kernel_code(A, 0) == want, (copy, self.kernel_code(A, 0))
        return A

    def kernel_code(self, A, side):
        return self.L.fs_matrix_spmv_kernel(A.h, side)

    def has_transpose(self, A):
        return self.L.fs_matrix_has_transpose(A.h)

    def ldsx_orderable(self, A, side):
        return 1 if self.L.fs_debug_ldsx_orderable(A.h, side) != 0 else 0

    def tiled_layout(self, A, side):
        v = self.L.fs_debug_tiled_layout(A.h, side)
        return v if v >= 0 else 0

    def spmm_plan(self, A, k, side):
        return self.L.fs_matrix_spmm_plan(A.h, k, side)

    def spmm_needs(self, A, k, side, creation):
        with self.options(**creation):
            return self.L.fs_debug_spmm_needs(A.h, k, side)

    def last_spmm_plan(self):
        return self.L.fs_debug_last_spmm_plan()

    def lazy_growth(self, A):
        n = 0
        for side in range(2 if self.has_transpose(A) else 1):
            if self.L.fs_debug_two_pass_rows8(A.h, side) >= 0:
                out = (self.C.c_ulonglong * 8)()
                assert self.L.fs_debug_two_pass_layout(A.h, side, out) == 0
                n += 2 * int(out[5])
        return n

    # -- the solvers ----
    def gram_diag(self, At, lam, d):
        self.capi.gram_diag(At, lam, d, self.stream())

    def solve(self, solver, A, At, x, b, lam=0.0, tol=1e-6, max_iter=0, precond=0, warm=False, diag=None, k=1, lams=(), ldx=0, null=(), m=1):
        """one solver call; null names arguments handed over as NULL.  {"iters": [...], "infos": [(iterations, converged, rnorm,
        bnorm), ...] or None} (fs_mscgn: info[i * k + j]); a negative status raises like every binding"""
        C, L, capi = self.C, self.L, self.capi
        pa, pt = None if "A" in null else A.h, None if "At" in null else At.h
        px, pb = None if "x" in null else x.data_ptr(), None if "b" in null else b.data_ptr()
        st = self.stream()
        if solver in ("cg", "cg2"):
            it = C.c_int(-1)
            capi.check(getattr(L, "fs_" + solver)(pa, pt, px, pb, lam, tol, C.byref(it), st), "fs_" + solver)
            return {"iters": [it.value], "infos": None}
        prm = capi.PcgParams(tol, max_iter, precond, int(warm), None if diag is None else diag.data_ptr())
        pp = None if "prm" in null else C.byref(prm)
        n = 1 if solver == "pcg" else max(k, 1) * max(m, 1) if solver == "mscgn" else max(k, 1)
        infos = (capi.PcgInfo * max(n, len(lams), 1))()
        # (room for every lambda a refused k or m could make the library look at)
        arr = None if "lambda" in null else (C.c_double * max(len(lams), 64))(*lams)
        if solver == "pcg":
            rc = L.fs_pcg(pa, pt, px, pb, lam, pp, infos, st)
        elif solver == "pcgn":
            rc = L.fs_pcgn(pa, pt, px, pb, k, lam, pp, infos, st)
        elif solver == "pcgn_lambdas":
            rc = L.fs_pcgn_lambdas(pa, pt, px, pb, k, arr, pp, infos, st)
        elif solver == "mscgn":
            rc = L.fs_mscgn(pa, pt, px, ldx, pb, k, m, arr, tol, max_iter, infos, st)
        else:
            rc = L.fs_mscg(pa, pt, px, ldx, pb, k, arr, tol, max_iter, infos, st)
        capi.check(rc, "fs_" + solver)
        out = [(i.iterations, i.converged, i.rnorm, i.bnorm) for i in list(infos)[:n]]
        return {"iters": [i[0] for i in out], "infos": out}

    def last_segments(self):
        return self.capi.pcgn_segments()

    def last_state(self, solver, n, m=1):
        """(st[] by name, the per-shift / per-column scalars by name) of the last solve, from the fs_debug_last_*_state hooks;
        fs_mscgn: per column (its st[] by name, its per-shift array by name), from fs_debug_last_mscgn_state(j)"""
        C, L = self.C, self.L
        if solver == "mscgn":
            L.fs_debug_last_mscgn_state.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int]
            cols = []
            for j in range(n):
                st, raw = np.full(M.CG_STATE_DOUBLES, np.nan), np.full(S.MAX_SHIFTS * S.MS_STRIDE, np.nan)
                assert L.fs_debug_last_mscgn_state(j, st.ctypes.data, raw.ctypes.data, raw.size) == m * S.MS_STRIDE
                cols.append((S.state_from_device(st), S.shifts_from_device(raw, m)))
            return None, cols
        L.fs_debug_last_cg_state.argtypes = [C.c_void_p]
        st = np.full(M.CG_STATE_DOUBLES, np.nan)
        assert L.fs_debug_last_cg_state(st.ctypes.data) == M.CG_STATE_DOUBLES
        if solver == "cg":
            return M.state_from_device(st, False), None
        if solver == "pcg":
            return P.state_from_device(st), None
        hook = L.fs_debug_last_mscg_state if solver == "mscg" else L.fs_debug_last_pcgn_state
        hook.argtypes = [C.c_void_p, C.c_int]
        raw = np.full(32 * 16, np.nan)
        stride = S.MS_STRIDE if solver == "mscg" else N.PN_STRIDE
        assert hook(raw.ctypes.data, raw.size) == n * stride
        if solver == "mscg":
            return S.state_from_device(st), S.shifts_from_device(raw, n)
        return P.state_from_device(st), N.state_from_device(raw, n)

    def poison_heap(self, sizes):
        return poison_heap(self.L, sizes)


def poison_heap(L, sizes):
    """fs_device_alloc every size a solve is about to ask for and two neighbours of it, fill with a quiet NaN tagged as poison,
    fs_device_free -- not through torch, whose allocator never hands memory back.  Then the probe: allocate the largest size
    again and count the doubles that still carry the poison.  (doubles seen, doubles probed).  L: capi.lib(); also the sharded
    suites' (tests/_dist_solvers.py)"""
    import torch
    torch.cuda.synchronize()
    want = sorted({n + d for n in sizes for d in (0, 2, 64)})
    host = np.full(max(want), guard_bits(POISON_TAG), np.int64)
    ptrs = []
    for n in want:
        p = L.fs_device_alloc(8 * n)
        assert p, "fs_device_alloc failed"
        ptrs.append(p)
        assert L.fs_copy_to_device(p, host.ctypes.data, 8 * n) == 0
    for p in reversed(ptrs):
        L.fs_device_free(p)
    n = max(sizes)
    p = L.fs_device_alloc(8 * n)
    assert p, "fs_device_alloc failed"
    back = np.zeros(n, np.int64)
    rc = L.fs_copy_to_host(back.ctypes.data, p, 8 * n)
    L.fs_device_free(p)
    assert rc == 0
    return int((back == host[0]).sum()), n
