"""Random operation walks on long-lived handles, with every vector inside guard zones (helper; no test in here).

A walk keeps two or three matrix handles alive and steps them in random interleaving through every legal call of
include/fastsparse_hip.h: products (one vector, k columns, A'A, in parts, host vectors), prepare / release_prepared,
release_csr / restore_csr / download, option flips, stream changes, handles destroyed and created mid-walk.  The data are the
exactly summable sets of tests/_exact.py, so ONE bar -- equality of bits -- serves every mode and every order of additions.

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
import contextlib
import re
import zlib

import numpy as np

import _exact as E

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
         "spmm_kernel": (0, 1, 2, 3), "spmm_wide": (0, -1, 1), "ata_kernel": (0, 2), "tiled_flags": (0, 4)}   # first value: default

# forced copies beyond the PATHS table of test_gpu_exact.py: the builder's own choice
AUTO = "auto"

OPS = {"spmv": 10, "spmv_t": 10, "spmm": 12, "spmm_t": 12, "ata": 6, "spmv_part": 12, "spmm_part": 5, "spmv_host": 3, "spmv_t_host": 3,
       "dev_then_host": 3, "prepare": 6, "release_prepared": 4, "prepare_roundtrip": 2, "release_csr": 5, "restore_csr": 5, "download": 2,
       "flip": 10, "stream": 4, "churn": 2, "build_transpose": 3, "bad_arg": 2}


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


TAGS = {}                           # tag -> name of the guarded vector (for the message of a guard value found in a sum)


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


class Walk:
    def __init__(self, backend, data, copy, seed, steps=150, upto=None, copies=None, kmax=17, nc=NC, nhandles=3, ata_cols=3):
        self.b, self.data, self.copy, self.seed = backend, data, copy, seed
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
                       "recovered": 0, "part_between": 0}

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
    def create(self, first=False, with_t=None, borrow=None):
        i = self.made
        self.made += 1
        d = self.data
        if first:
            copy, pattern = self.copy, False
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
            H.A = self.b.create(d, copy, arrays, borrow)
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
        gone = set(self.ks) if k == 0 else {2, 3} if k in (2, 3) else {k}
        for side in (0, 1) if m.has_t else (0,):
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
                self.handles = []

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

    def create(self, d, copy, arrays, borrow):
        rp, cc, vv = arrays
        if not borrow:
            rp, cc, vv = (None if a is None else self.mem.const(a) for a in arrays)
        A = self.capi.Matrix.from_csr(d.nrow, d.ncol, rp, cc, vv, borrow=borrow)
        if copy != AUTO:
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
