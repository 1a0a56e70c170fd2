"""The lifecycle harness (tests/_lifecycle.py) has teeth, shown without a GPU.

A numpy stand-in for the library -- the method names of capi.Matrix, vectors as numpy views into guarded arenas, products by
bincount over the COO entries (exact on exactly summable data, whatever the order), the status rules of the header, the
bookkeeping the walk asks about -- runs the SAME walk code as the GPU tests.  The honest stand-in passes; each injected fault makes
a walk fail at the step where it first matters, with a message that names it; and the operation mix of the seeds the GPU test uses
is checked, so that a generator that stops reaching an operation is a failing test and not a silent loss."""
import contextlib

import numpy as np
import pytest

import _cg_model as M
import _lifecycle as LC
import _pcg_model as P

COPIES = ["stream", "two-pass", "two-pass one-byte", "long rows", "lds-staged", "tiled cut rows", LC.AUTO]
CODES = {"stream": 1, "two-pass": 7, "two-pass one-byte": 7, "long rows": 7, "lds-staged": 8, "tiled cut rows": 6, LC.AUTO: 1}
DEFAULTS = {"reproducible": 0, "strict_order": 0, "cg_fixed_order": 1, "spmv_kernel": 0, "spmm_kernel": 0, "spmm_wide": 0, "ata_kernel": 0,
            "tiled_flags": 0, "binning": 1, "pcgn_compact": 0, "pcgn_kernel": 0}
SEEDS = (1, 2)                      # the seeds of tests/test_gpu_lifecycle.py
STEPS = 150


class StandInError(RuntimeError):
    pass


def _raise(rc, what):
    raise StandInError(f"{what} failed ({rc}): stand-in")


def _where(v):
    """(the allocation a view lies in, its offset in doubles)"""
    base = v
    while base.base is not None:
        base = base.base
    base = base.view(np.float64)
    return base, (v.ctypes.data - base.ctypes.data) // 8


class StandInMatrix:
    def __init__(self, lib, d, code, borrow):
        self.lib, self.d, self.h = lib, d, True
        self.code = [code, code]
        self.has_t = False
        self.released = [False, False]
        self.owned = [not borrow, True]
        self.slot = [set(), set()]              # k-column two-pass copies built: 2 (serves k = 2, 3), 4
        self.scratch_k = [0, 0]                 # columns the column-major scratch of the LDS-staged copy holds
        self.choice = [dict(), dict()]
        self.part_plans = [[], []]
        self.last = {}
        self.stale = {}

    # -- bookkeeping ----
    def _o(self):
        return self.lib.opt

    def kernel_code(self, side):
        o, kept = self._o(), self.code[side]
        if not o["strict_order"] and kept >= 6 and o["spmv_kernel"] in (0, kept):
            return kept
        return 2 if o["spmv_kernel"] == 2 else 1

    def spmm_plan(self, k, transposed=False):
        side, o = int(transposed), self._o()
        kept, want = self.code[side], o["spmm_kernel"]
        if o["strict_order"] or want == 1:
            return 1
        if kept == 7 and o["spmv_kernel"] in (0, 7):
            if 2 <= k <= 4 and (4 if k == 4 else 2) in self.slot[side]:
                return 2
            return 3 if (k <= 3 or want == 3) else 1
        if kept == 8 and k <= 16 and o["spmv_kernel"] in (0, 8):
            if self.scratch_k[side] >= k:
                return 1 if (want == 0 and k > 2 and self.choice[side].get(k) == 2) else 5
            return 6 if k <= 2 else 1
        if kept == 6 and k <= 2 and o["spmv_kernel"] in (0, 6):
            return 7
        return 1

    def spmm_needs(self, k, side):
        o, n = self._o(), 0
        if k < 2:
            return 0
        if (self.code[side] == 7 and 2 <= k <= 4 and not o["strict_order"] and o["spmm_kernel"] in (0, 2) and o["spmv_kernel"] in (0, 7)
                and (4 if k == 4 else 2) not in self.slot[side]):
            n |= 1
        if self.code[side] == 8 and k <= 16 and not o["strict_order"] and o["spmm_kernel"] != 1 and o["spmv_kernel"] in (0, 8):
            if self.scratch_k[side] < k:
                n |= 4
            if k > 2 and o["spmm_kernel"] == 0 and k not in self.choice[side]:
                n |= 2                                              # sweeps timed against the row kernel: reads the plain CSR
        return n

    def device_bytes(self):
        b = [0, 0, 0]
        for s in (0, 1) if self.has_t else (0,):
            b[0] += 0 if self.released[s] else (12 * self.d.nnz if self.owned[s] else 0) + 64
            b[1] += 20 * self.d.nnz if self.code[s] >= 6 else 0
            b[2] += sum(10 * kk * self.d.nnz for kk in self.slot[s]) + 8 * self.scratch_k[s] * (self.d.nrow + self.d.ncol)
        return tuple(b)

    # -- the products ----
    def _sides(self, side):
        d = self.d
        return (d.rows, d.cols, d.nrow, d.ncol) if side == 0 else (d.cols, d.rows, d.ncol, d.nrow)

    def _mul(self, y, x, side, k, r0=0, r1=None):
        lib = self.lib
        out_idx, in_idx, n_out, n_in = self._sides(side)
        w = 1.0 if self.d.vals is None else self.d.vals
        X = np.array(x).reshape(n_in, k)
        key = (side, k, x.ctypes.data)
        if True:
            G = X[in_idx]
            if lib.fault == "guard value read" and n_in > 0:
                base, off = _where(x)
                hit = in_idx == 0
                if hit.any():
                    lib.fired()
                    G = G.copy()
                    G[hit, 0] = base[off - 1]                      # one double in front of x instead of x[0]
            Y = np.stack([np.bincount(out_idx, weights=w * G[:, j], minlength=n_out) for j in range(k)], 1)
        if lib.fault == "cached output":                            # the same input pointer again: the output of last time
            old = self.last.get(key)
            self.last[key] = Y
            if old is not None and not np.array_equal(old.view(np.int64), Y.view(np.int64)):
                lib.fired()
                Y = old
        if lib.fault == "x modified" and lib.calls >= 3 and n_in > 2:
            lib.fired()
            x[n_in // 2] = 1.5
        r1 = n_out if r1 is None else r1
        y.reshape(n_out, k)[r0:r1] = Y[r0:r1]
        if r1 == n_out and r0 == 0:
            base, off = _where(y)
            if lib.fault == "store past y" and k == 1 and lib.calls >= 3:
                lib.fired()
                base[off + y.size] = 1.0
            if lib.fault == "store before Y" and k > 1 and y.ctypes.data % 16 == 8:
                lib.fired()
                base[off - 1] = Y[0, 0]
        lib.calls += 1

    def _single(self, side, what):
        if side and not self.has_t:
            _raise(LC.FS_ERR_NO_TRANSPOSE, what)
        if self.released[side] and self.kernel_code(side) < 6:
            if self.lib.fault == "released answers" and self._o()["strict_order"]:
                self.lib.fired()
                return
            _raise(LC.FS_ERR_RELEASED, what)

    def spmv(self, y, x, stream=None, transposed=False):
        if y is None or x is None:
            _raise(LC.FS_ERR_ARG, "fs_spmv")
        self._single(int(transposed), "fs_spmv")
        self._mul(y, x, int(transposed), 1)

    def spmv_host(self, y, x, transposed=False):
        self.spmv(y, x, None, transposed)

    def _multi(self, Y, X, k, side):
        if side and not self.has_t:
            _raise(LC.FS_ERR_NO_TRANSPOSE, "fs_spmm")
        plan = self.spmm_plan(k, side)
        self.lib.last_plan = plan
        if plan == 1 and self.released[side]:
            _raise(LC.FS_ERR_RELEASED, "fs_spmm")
        return plan

    def spmm(self, Y, X, k, stream=None, transposed=False):
        if k < 1:
            _raise(LC.FS_ERR_ARG, "fs_spmm")
        side = int(transposed)
        plan = self._multi(Y, X, k, side)
        self.lib.last_plan = plan
        self._mul(Y, X, side, k)
        if plan == 5:
            # the product goes through column-major scratch: columns the scratch has no room for come out stale
            n_out = self._sides(side)[2]
            cap = self.stale.get(side)
            if cap is not None and cap < k:
                self.lib.fired()
                Y.reshape(n_out, k)[:, cap:] = 0.0

    def ata(self, y, x, tmp, stream=None):
        o = self._o()
        if o["ata_kernel"] == 2 and not o["strict_order"] and not o["reproducible"]:
            if self.released[0] and self.code[0] != 8:
                _raise(LC.FS_ERR_RELEASED, "fs_ata_mul")
            self._mul(tmp, x, 0, 1)                                 # (tmp is the caller's scratch: the fused form may use it)
            self._mul(y, tmp, 1, 1)
            return
        self.build_transpose()
        self.spmv(tmp, x)
        self.spmv(y, tmp, None, True)

    # -- in parts ----
    def _cuts(self, side, nparts, kind):
        n = self._sides(side)[2]
        if kind < 6 or nparts < 2:
            return [0] + [n] * nparts
        return [min(n, (n * p // nparts) // 32 * 32) for p in range(nparts)] + [n]

    def _bounds(self, side, nparts):
        kind = self.kernel_code(side)
        plans = self.part_plans[side]
        for n, kd, rows in plans:
            if n == nparts and kd == kind:
                return rows
        rows = self._cuts(side, nparts, kind)
        if len(plans) >= 8:
            old = plans.pop(0)
            if self.lib.fault == "evicted cuts" and kind >= 6 and nparts > 1:
                self.evicted = (nparts, kind, old[2])
        plans.append((nparts, kind, rows))
        return rows

    def part_rows(self, nparts, transposed=False, k=1):
        side = int(transposed)
        if nparts < 1 or nparts > 64 or k < 1:
            _raise(LC.FS_ERR_ARG, "fs_spmm_part_rows")
        if side and not self.has_t:
            _raise(LC.FS_ERR_NO_TRANSPOSE, "fs_spmm_part_rows")
        if k == 1:
            return list(self._bounds(side, nparts))
        cut = k in (2, 4) and self.spmm_plan(k, side) == 2
        return self._cuts(side, nparts, 7 if cut else 1)

    def spmv_part(self, y, x, part, nparts, stream=None, transposed=False):
        side = int(transposed)
        if nparts < 1 or nparts > 64 or part < 0 or part >= nparts:
            _raise(LC.FS_ERR_ARG, "fs_spmv_part")
        if side and not self.has_t:
            _raise(LC.FS_ERR_NO_TRANSPOSE, "fs_spmv_part")
        rows = self._bounds(side, nparts)
        ev = getattr(self, "evicted", None)
        if ev and ev[:2] == (nparts, self.kernel_code(side)):       # the fault: the cuts of the plan that was pushed out
            old = ev[2]
            wrong = [old[min(p, len(old) - 2)] for p in range(nparts)] + [old[-1]]
            if wrong != rows:
                self.lib.fired()
                rows = wrong
        if rows[1] == rows[-1] and nparts > 1 or nparts == 1:
            if part == 0:
                self._single(side, "fs_spmv_part")
                self._mul(y, x, side, 1)
            return
        self._mul(y, x, side, 1, rows[part], rows[part + 1])

    def spmm_part(self, Y, X, k, part, nparts, stream=None, transposed=False):
        side = int(transposed)
        if k < 1 or nparts < 1 or nparts > 64 or part < 0 or part >= nparts:
            _raise(LC.FS_ERR_ARG, "fs_spmm_part")
        rows = self.part_rows(nparts, transposed, k)
        plan = self._multi(Y, X, k, side) if part == 0 or rows[1] != rows[-1] else None
        if rows[1] == rows[-1]:
            if part == 0:
                self.lib.last_plan = plan
                self._mul(Y, X, side, k)
            return
        self._mul(Y, X, side, k, rows[part], rows[part + 1])

    # -- one-time work, release, restore ----
    def build_transpose(self, stream=None):
        if self.has_t:
            return
        if self.released[0]:
            _raise(LC.FS_ERR_RELEASED, "fs_matrix_build_transpose")
        self.has_t = True

    def prepare(self, k, stream=None, transposed=False):
        side = int(transposed)
        if k < 1:
            _raise(LC.FS_ERR_ARG, "fs_matrix_prepare")
        if side and not self.has_t:
            _raise(LC.FS_ERR_NO_TRANSPOSE, "fs_matrix_prepare")
        needs = self.spmm_needs(k, side)
        if needs & 1:
            if self.released[side]:
                _raise(LC.FS_ERR_RELEASED, "fs_matrix_prepare")
            self.slot[side].add(4 if k == 4 else 2)
        if needs & 4:
            if self.lib.fault == "scratch not grown" and 0 < self.scratch_k[side] < k:
                self.stale[side] = self.scratch_k[side]
            self.scratch_k[side] = max(self.scratch_k[side], k)
        if needs & 2:
            if self.released[side]:
                _raise(LC.FS_ERR_RELEASED, "fs_matrix_prepare")
            self.choice[side][k] = 1

    def release_prepared(self, k=0):
        n = 0
        if self.lib.fault == "release_prepared keeps":
            if any((k in (0, 2, 3) and 2 in self.slot[s]) or (k in (0, 4) and 4 in self.slot[s]) or (k == 0 and self.scratch_k[s]) for s in (0, 1)):
                self.lib.fired()
            return 1
        for s in (0, 1):
            if k in (0, 2, 3) and 2 in self.slot[s]:
                self.slot[s].discard(2)
                n += 1
            if k in (0, 4) and 4 in self.slot[s]:
                self.slot[s].discard(4)
                n += 1
            if self.scratch_k[s] and (k == 0 or 2 <= k <= 16):
                self.choice[s].pop(k, None)
                if k == 0 or not self.choice[s]:
                    self.scratch_k[s], self.choice[s] = 0, {}
                    self.stale.pop(s, None)
                    n += 1
        return n

    def release_csr(self):
        n = 0
        for s in (0, 1) if self.has_t else (0,):
            if self.code[s] >= 6 and not self.released[s]:
                self.released[s] = True
                n += 1
        return n

    def restore_csr(self, row_ptr, cols, vals=None, transposed=False, borrow=False):
        side = int(transposed)
        if row_ptr is None or (side and not self.has_t):
            _raise(LC.FS_ERR_ARG, "fs_matrix_restore_csr")
        if self.released[side]:
            self.released[side] = False
            self.owned[side] = not borrow

    def download(self, transposed=False):
        side = int(transposed)
        if side and not self.has_t:
            _raise(LC.FS_ERR_NO_TRANSPOSE, "fs_matrix_download")
        if self.released[side]:
            _raise(LC.FS_ERR_RELEASED, "fs_matrix_download")
        rp, cc, vv = LC.refs_of(self.d, self.lib.nc).csr[side]
        return rp.copy(), cc.copy(), None if vv is None else vv.copy()

    def close(self):
        self.h = None


class StandIn:
    """the backend of a walk: a library of StandInMatrix handles with process-wide options and, optionally, one injected fault"""
    Error = StandInError

    def __init__(self, fault=None, nc=LC.NC):
        self.fault, self.nc = fault, nc
        self.opt = dict(DEFAULTS)
        self.mem = self.hostmem = LC.NumpyMem()
        self.last_plan = 0
        self.calls = 0
        self.step = -1
        self.first_fired = None
        self.cur = 0
        self.pool = np.zeros(1)

    def fired(self):
        if self.first_fired is None:
            self.first_fired = self.step

    def copies(self):
        return list(COPIES)

    def creation_options(self, copy):
        return {}

    def get_option(self, name):
        return self.opt[name]

    def set_option(self, name, value):
        self.opt[name] = value

    @contextlib.contextmanager
    def options(self, **kw):
        old = {k: self.opt[k] for k in kw}
        try:
            self.opt.update(kw)
            yield
        finally:
            self.opt.update(old)

    @contextlib.contextmanager
    def walk_scope(self):
        yield

    def begin_step(self, i):
        self.step = i

    def stream(self):
        return self.cur

    def stream_index(self):
        return self.cur

    def switch_stream(self):
        self.cur ^= 1

    def create(self, d, copy, arrays, borrow, must=True):
        return StandInMatrix(self, d, CODES[copy], borrow)

    # -- the solvers: the status rules of the header, then the models ----
    def gram_diag(self, At, lam, d):
        if At.released[0]:
            _raise(LC.FS_ERR_RELEASED, "fs_gram_diag")
        d[...] = P.gram_diag(At.d.system.t_csr, lam)

    def _ready(self, Mx, k, what):
        """a product of the solve would read plain arrays that were released"""
        if Mx.released[0] and (Mx.kernel_code(0) < 6 if k == 1 else Mx.spmm_plan(k, 0) in (LC.ROW_PLAN, LC.MFMA_PLAN)):
            _raise(LC.FS_ERR_RELEASED, what)

    def solve(self, solver, A, At, x, b, lam=0.0, tol=1e-6, max_iter=0, precond=0, warm=False, diag=None, k=1, lams=(), ldx=0, null=(), m=1):
        what, fault, answers = "fs_" + solver, self.fault, False
        if null or (At is not None and A is not None and (At.d.nrow, At.d.ncol) != (A.d.ncol, A.d.nrow)):
            _raise(LC.FS_ERR_ARG, what)
        F = A.d.ncol
        if solver == "pcgn" and not 1 <= k <= 32 or solver == "mscg" and (not 1 <= k <= 16 or ldx < F or not np.isfinite(lams).all()):
            _raise(LC.FS_ERR_ARG, what)
        if solver == "pcgn_lambdas" and (not 1 <= k <= 32 or not np.isfinite(lams[:k]).all()):
            _raise(LC.FS_ERR_ARG, what)
        if solver == "mscgn" and (not 1 <= k <= 32 or not 1 <= m <= 16 or ldx < F * k or not np.isfinite(lams[:m]).all()):
            _raise(LC.FS_ERR_ARG, what)
        pcgs = ("pcg", "pcgn", "pcgn_lambdas")
        if solver in pcgs + ("mscg", "mscgn") and not tol >= 0.0 or solver in pcgs and (precond not in (0, 1, 2) or precond == 2 and diag is None):
            _raise(LC.FS_ERR_ARG, what)
        if precond == P.PRECOND_JACOBI and At.released[0]:
            if fault == "jacobi on a released At zeroes x":
                self.fired()
                x[...] = 0.0
            if fault != "jacobi on a released At answers":
                _raise(LC.FS_ERR_RELEASED, what)
            answers = True
        kk = 2 if solver == "cg2" else k if solver in LC.K_COLUMNS else 1
        if kk >= 2:
            unprepared = fault == "pcgn leaves k unprepared" and ((A.spmm_needs(kk, 0) | At.spmm_needs(kk, 0)) & 5)
            if fault != "pcgn leaves k unprepared":
                A.prepare(kk)
                At.prepare(kk)
        self._ready(A, kk, what)
        self._ready(At, kk, what)
        if kk >= 2 and unprepared or answers:
            self.fired()
        usable = []                                         # option "pcgn_compact": the rungs below k, settled before x is written
        if solver in LC.NARROWING and self.opt["pcgn_compact"]:
            for w in (16, 8, 4, 2, 1):
                if w >= k:
                    continue
                try:
                    if w >= 2:
                        A.prepare(w)
                        At.prepare(w)
                    self._ready(A, w, what)
                    self._ready(At, w, what)
                except StandInError as ex:                  # a refused width is silent
                    assert f"({LC.FS_ERR_RELEASED})" in str(ex), ex
                    if fault == "a refused width is reported as an error":
                        self.fired()
                        raise
                    continue
                usable.append(w)
        ps = A.d.system
        x0 = np.array(x) if warm else None
        lams = list(lams) or None
        if fault == "pcgn_lambdas takes lambda[0] for every column" and solver == "pcgn_lambdas" and any(
                l != lams[0] and np.asarray(b).reshape(F, k)[:, j].any() for j, l in enumerate(lams)):
            self.fired()
            lams = [lams[0]] * k
        r = LC.solve_model(ps, solver, np.array(b), lam, tol, max_iter, precond, x0, None if diag is None else np.array(diag), lams)
        pool, self.pool = self.pool, np.zeros(1)            # the work space of this solve: whatever its last owner left
        if solver == "mscg":
            for i in range(k):
                x[i * ldx:i * ldx + F] = r.x[i]
            if fault == "mscg writes into the gap" and ldx > F and k > 1:
                self.fired()
                x[F] = 0.0
        elif solver == "mscgn":
            for i in range(m):
                x[i * ldx:i * ldx + F * k] = np.ascontiguousarray(r.x[i]).reshape(-1)
            if fault == "mscgn writes into the gap between panels" and ldx > F * k and m > 1:
                self.fired()
                x[F * k + 1] = 0.0
            if fault == "mscgn writes a frozen pair" and k >= 2:
                self.fired()
                x[(m - 1) * ldx:(m - 1) * ldx + F * k].reshape(F, k)[3, k // 2] = -0.0      # (the zero column: its pairs are frozen from the start)
        else:
            x[...] = np.ascontiguousarray(r.x).reshape(-1)
        reads = {"work space read before it is written": True, "pcgn_lambdas reads work space before it is written": solver == "pcgn_lambdas",
                 "mscgn reads work space before it is written": solver == "mscgn"}.get(fault, False)
        if reads and x[0] != 0.0 and pool.view(np.int64)[0] != 0:
            self.fired()
            x[0] = x[0] + pool[0]
        if fault == "pcgn writes a frozen column" and solver == "pcgn" and k >= 2:
            self.fired()
            x.reshape(F, k)[3, k // 2] = -0.0               # (the zero column: frozen from the start)
        if solver in LC.NARROWING:
            segs = self.segments = LC.PM.plan(k, usable, r.iters, ["rsq" not in st for st in r.extra], max_iter or F)
            narrow = [sg for sg in segs if sg[1] < k]
            if fault == "narrowing writes a column that was left behind" and narrow:
                j = min(j for j in range(k) if not narrow[-1][2] >> j & 1)
                self.fired()
                col = x.reshape(F, k)[:, j]
                col[3] = -0.0 if col.view(np.int64)[3] != LC.PREFILLS["-0.0"] else 1.0
            padded = any(w > bin(mask).count("1") for _, w, mask in narrow)
            if fault == "narrowing leaves a padding column unzeroed" and padded and x[0] != 0.0 and pool.view(np.int64)[0] != 0:
                self.fired()
                x[0] = x[0] + pool[0]
        base, off = _where(x)
        if fault == "solver stores past x" and self.calls >= 3:
            self.fired()
            base[off + x.size] = 1.0
        if fault == "solver writes into b" and self.calls >= 3:
            self.fired()
            b[b.size // 2] = 1.5
        if fault == "scope left on" and self.calls >= 3 and not self.opt["reproducible"]:
            self.fired()
            self.opt["reproducible"] = 1
        self.calls += 1
        infos = None if r.infos is None else [(i.iterations, i.converged, i.rnorm, i.bnorm) for i in r.infos]
        return {"iters": list(r.iters), "infos": infos}

    def last_segments(self):
        return list(self.segments)

    def last_state(self, solver, n, m=1):
        return None                                         # (the stand-in's scalars ARE the model's)

    def poison_heap(self, sizes):
        self.pool = np.full(1, LC.guard_bits(LC.POISON_TAG), np.int64).view(np.float64)
        return 1, 1

    def kernel_code(self, A, side):
        return A.kernel_code(side)

    def has_transpose(self, A):
        return int(A.has_t)

    def ldsx_orderable(self, A, side):
        return 1

    def tiled_layout(self, A, side):
        return 0

    def spmm_plan(self, A, k, side):
        return A.spmm_plan(k, side)

    def spmm_needs(self, A, k, side, creation):
        return A.spmm_needs(k, side)

    def last_spmm_plan(self):
        p, self.last_plan = self.last_plan, 0
        return p

    def lazy_growth(self, A):
        return 0


@pytest.fixture(scope="module")
def sets():
    return {n: LC.data_sets()[n] for n in LC.SET_NAMES}


@pytest.fixture(scope="module")
def gpu_walks(sets):
    """the walks of tests/test_gpu_lifecycle.py (data set x copy x seed) on the honest stand-in, run once"""
    return [LC.run_walk(StandIn(), sets[name], copy, seed, steps=STEPS) for name in sets for copy in COPIES for seed in SEEDS]


def test_the_honest_stand_in_passes_walks_of_every_data_set_and_copy(sets, gpu_walks):
    assert len(gpu_walks) == len(sets) * len(COPIES) * len(SEEDS) and all(len(w.log) > STEPS for w in gpu_walks)
    for seed in (3, 4, 5, 6):
        LC.run_walk(StandIn(), sets["subnormal"], "lds-staged", seed, steps=STEPS)


# fault -> (the kind of failure the message must carry, words it must contain)
FAULTS = {
    "store past y": (("guard",), "1 double(s) past its end"),
    "store before Y": (("guard",), "1 double(s) before it"),
    "x modified": (("input modified",), "in vector of"),
    "guard value read": (("guard value read",), "a guard value of"),
    "evicted cuts": (("rows below the cut", "rows above the cut"), "cuts"),
    "scratch not grown": (("not exact",), "plan 5"),
    "released answers": (("status",), "FS_ERR_RELEASED"),
    "release_prepared keeps": (("release_prepared", "device bytes"), "release_prepared("),
    "cached output": (("not exact", "rows below the cut"), "differ"),
    # the solvers on the pairs
    "solver stores past x": (("guard",), "1 double(s) past its end"),
    "solver writes into b": (("input modified",), "b of the solvers"),
    "jacobi on a released At answers": (("status",), "FS_ERR_RELEASED"),
    "jacobi on a released At zeroes x": (("x written",), "wrote to x all the same"),
    "pcgn leaves k unprepared": (("bookkeeping", "status"), "fs_"),
    "pcgn writes a frozen column": (("not exact",), "fs_pcgn"),
    "scope left on": (("option", "bookkeeping"), "reproducible"),
    "work space read before it is written": (("guard value read",), "a guard value of poison"),
    "mscg writes into the gap": (("gap written",), "a gap between the vectors of X"),
    # fs_pcgn_lambdas and fs_mscgn
    "mscgn writes into the gap between panels": (("gap written",), "a gap between the vectors of X"),
    "mscgn writes a frozen pair": (("not exact",), "fs_mscgn"),
    "pcgn_lambdas takes lambda[0] for every column": (("not exact",), "fs_pcgn_lambdas"),
    "pcgn_lambdas reads work space before it is written": (("guard value read",), "a guard value of poison"),
    "mscgn reads work space before it is written": (("guard value read",), "a guard value of poison"),
    # option "pcgn_compact"
    "narrowing writes a column that was left behind": (("not exact",), "fs_pcgn"),
}
# faults that need several rare things at once (option "pcgn_compact" on, a panel with padding right behind the poison; a released
# pair that still solves k and cannot prepare a rung): no seeded walk of 150 steps meets them twice, so a driven walk does --
# fault -> (kind, words, the step of DRIVEN at which it first matters)
DRIVEN_FAULTS = {
    "narrowing leaves a padding column unzeroed": (("guard value read",), "a guard value of poison", 4),
    "a refused width is reported as an error": (("status",), "FS_ERR_RELEASED", 3),
}
RARE = ("jacobi on a released At answers", "jacobi on a released At zeroes x", "pcgn leaves k unprepared")     # (need a released pair)


@pytest.mark.parametrize("fault", list(FAULTS))
def test_an_injected_fault_fails_the_walk_at_the_step_where_it_first_matters(sets, fault):
    kind, words = FAULTS[fault]
    copy = {"scratch not grown": "lds-staged", "evicted cuts": "two-pass"}.get(fault, "two-pass")
    kw = {}
    if fault in ("scratch not grown", "evicted cuts", "release_prepared keeps"):     # (rare orders of product operations: no solver pairs)
        kw = dict(copies=[copy], nhandles=2, solvers=False)
    elif fault in RARE:
        kw = dict(copies=[copy], nhandles=1)
    caught = 0
    for seed in range(1, 41 if fault in RARE else 13):
        if caught >= 2 and seed > 12:
            break
        lib = StandIn(fault)
        try:
            LC.run_walk(lib, sets["wide_range"], copy, seed, steps=STEPS, **kw)
        except LC.WalkFailure as ex:
            assert lib.first_fired is not None, (fault, seed, str(ex))
            assert ex.kind in kind and words in str(ex), (fault, seed, ex.kind, str(ex)[:600])
            assert ex.step == lib.first_fired, (fault, seed, ex.step, lib.first_fired, str(ex)[:600])
            assert f"seed {seed}" in str(ex) and f"step {ex.step}" in str(ex) and "last operations" in str(ex)
            # the replay of the failing prefix fails at the same step, one step less passes
            with pytest.raises(LC.WalkFailure) as again:
                LC.run_walk(StandIn(fault), sets["wide_range"], copy, seed, steps=STEPS, upto=ex.step + 1, **kw)
            assert again.value.step == ex.step
            caught += 1
        else:
            assert lib.first_fired is None, (fault, seed, "the fault fired at step", lib.first_fired, "and the walk passed")
    assert caught >= 2, (fault, caught)


def _driven_walk(lib, sets):
    """pairs on LDS-staged copies: 5 columns before and, under option "pcgn_compact", after fs_matrix_release_csr -- the released pair
    still multiplies 5 columns (its sweeps were timed before the release) and 2, but cannot prepare 4: a refused width, silently,
    and the solve is FS_OK on one segment; then on another pair 17 columns right behind the poison (15 live ones in a panel of
    16: a padding column)"""
    w = LC.Walk(lib, sets["wide_range"], "lds-staged", seed=1, steps=0, copies=["lds-staged"])

    def step(f, *a, **kw):
        w.step += 1
        lib.begin_step(w.step)
        return f(*a, **kw)

    with w.session():
        w.create(first=True)
        pair, other = w.create_pair("exact"), w.create_pair("exact", valued=True)
        names = [c[1] for c in LC.exact_cases(pair.ps.fam) if c[0] == "pcgn"]
        rc, _ = step(w.exact_solve, pair.A, "pcgn", poison=False, pick=names.index("fs_pcgn k 5 none cold"))   # 0
        assert rc == LC.FS_OK
        step(w.op_release_csr, pair.A)                                                                        # 1
        w.op_release_csr(pair.At)
        step(w.flip, "pcgn_compact", 1)                                                                       # 2
        rc, _ = step(w.exact_solve, pair.A, "pcgn", poison=True, pick=names.index("fs_pcgn k 5 none cold"))    # 3
        assert rc == LC.FS_OK and "usable widths [2, 1], segments [(0, 5, 31)]" in w.log[-1], w.log[-1]
        rc, _ = step(w.exact_solve, other.A, "pcgn", poison=True, pick=names.index("fs_pcgn k 17 none cold"))  # 4
        assert rc == LC.FS_OK and w.counts["repacked"] == 1 and "segments [(0, 16," in w.log[-1], w.log[-1]
    return w


def test_the_honest_stand_in_passes_the_driven_walk(sets):
    _driven_walk(StandIn(), sets)


@pytest.mark.parametrize("fault", list(DRIVEN_FAULTS))
def test_a_rare_narrowing_fault_fails_the_driven_walk_at_the_step_where_it_first_matters(sets, fault):
    kind, words, at = DRIVEN_FAULTS[fault]
    lib = StandIn(fault)
    with pytest.raises(LC.WalkFailure) as ex:
        _driven_walk(lib, sets)
    assert ex.value.kind in kind and words in str(ex.value), (fault, ex.value.kind, str(ex.value)[:600])
    assert ex.value.step == lib.first_fired == at, (fault, ex.value.step, lib.first_fired, at)


def test_the_operation_mix_reaches_everything(sets, gpu_walks):
    """over the walks the GPU test runs: every operation, every predicted status, more than eight distinct nparts on one handle,
    every k on both sides, a host-vector product directly behind a device-vector product, restores copied and borrowed"""
    ops, status, ks, nparts, behind, restore, recovered, between = {}, {}, [set(), set()], 0, 0, set(), 0, 0
    assert set(LC.GPU_SET_NAMES) <= set(sets)
    for w in gpu_walks:
        if w.data.name not in LC.GPU_SET_NAMES:
            continue
        c = w.counts
        for k, v in c["ops"].items():
            ops[k] = ops.get(k, 0) + v
        for k, v in c["status"].items():
            status[k] = status.get(k, 0) + v
        for s in (0, 1):
            ks[s] |= c["k"][s]
        nparts = max([nparts] + list(c["nparts"].values()))
        behind += c["host_behind_device"]
        restore |= c["restore"]
        recovered += c["recovered"]
        between += c["part_between"]
        assert sum(c["ops"].values()) == STEPS
    missing = [o for o in LC.OPS if ops.get(o, 0) < 5]
    assert not missing, (missing, ops)
    for s in (LC.FS_OK, LC.FS_ERR_ARG, LC.FS_ERR_NO_TRANSPOSE, LC.FS_ERR_RELEASED):
        assert status.get(s, 0) >= 10, status
    assert ks[0] == set(LC.KS) and ks[1] == set(LC.KS), ks
    assert nparts > 8, nparts
    assert behind >= 5 and restore == {"copied", "borrowed"} and recovered >= 10 and between >= 5, (behind, restore, recovered, between)


def test_guarded_vectors_sit_where_they_say(sets):
    mem = LC.NumpyMem()
    g = LC.Guarded(mem, "probe", 100)
    for off8 in (0, 1):
        v = g.place(37, off8)
        assert v.ctypes.data % 16 == 8 * off8 and g.lo >= LC.GUARD and g.store.size - g.hi >= LC.GUARD
        assert g.guards_ok() and LC.guard_tag(g.store.view(np.int64)[0]) == g.tag and np.isnan(g.store[0])
        g.store[g.hi] = 0.0
        assert not g.guards_ok() and "1 double(s) past its end" in g.first_broken()
        g.place(37, off8)
        g.store[g.lo - 1] = 0.0
        assert not g.guards_ok() and "1 double(s) before it" in g.first_broken()
    assert LC.guard_tag(np.float64(np.nan).view(np.int64)) is None


# ---- the solvers on the pairs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("valued", (False, True), ids=("binary", "valued"))
def test_the_exact_family_is_exact_in_any_order_of_additions(valued):
    """every solve the walks run on the exact family, by each solver's model, once with the device's reduction tree and once with
    serial sums: identical bits in x, the counts and the info -- the solves can run in whatever mode a walk is in.  And they are
    the solves they are meant to be: converged at iteration 0, x = b / 2^e"""
    ps = LC.pair_system("exact", valued)
    fam = ps.fam
    cases = LC.exact_cases(fam)
    assert {c[0] for c in cases} == set(LC.EXACT_ONLY)
    assert {kw["b"].size // fam.F for sv, _, kw in cases if sv == "pcgn"} == set(LC.PCGN_KS)
    assert {kw["b"].size // fam.F for sv, _, kw in cases if sv == "pcgn_lambdas"} == set(LC.PCGN_KS)
    assert {(kw["b"].size // fam.F, len(kw["lams"])) for sv, _, kw in cases if sv == "mscgn"} == {(k, m) for k in LC.MSCGN_KS for m in (1, 3, 8)}
    assert all(len(set(kw["lams"])) < len(kw["lams"]) for sv, _, kw in cases if sv in ("pcgn_lambdas", "mscgn") and len(kw["lams"]) >= 3), "duplicates"
    assert fam.c == 2.0 ** int(np.log2(fam.c)) and all(np.log2(fam.d + l) % 1 == 0 for ls in fam.ladders.values() for l in ls)
    assert fam.ladders["m16"].count(min(fam.ladders["m16"])) >= 2 and len(fam.ladders["m16"]) == 16
    assert np.array_equal(P.gram_diag(ps.t_csr, fam.s.lam), np.full(fam.F, fam.c)) and (valued == (fam.s.vals is not None))
    for solver, what, kw in cases:
        dev = LC.solve_model(ps, solver, lam=fam.s.lam, tol=fam.s.tol, **kw)
        ser = LC.solve_model(ps, solver, lam=fam.s.lam, tol=fam.s.tol, tree="serial", **kw)
        assert M.same_bits(dev.x, ser.x).all() and np.isfinite(dev.x).all(), (what, "x depends on the order of the additions")
        assert dev.iters == ser.iters == [0] * len(dev.iters), (what, dev.iters, ser.iters)
        for a, b in zip(dev.infos or [], ser.infos or []):
            assert (a.iterations, a.converged) == (b.iterations, b.converged) == (0, 1), (what, a, b)
            assert M.same_bits(a.rnorm, b.rnorm)[0] and M.same_bits(a.bnorm, b.bnorm)[0], (what, a, b)
        B = kw["b"]
        if solver == "mscg":
            want = np.stack([B / (fam.d + l) for l in kw["lams"]])
        elif solver == "mscgn":
            want = np.stack([B.reshape(fam.F, -1) / (fam.d + l) for l in kw["lams"]])
        elif solver == "pcgn_lambdas":
            want = B.reshape(fam.F, -1) / (fam.d + np.array(kw["lams"]))[None, :]
        else:
            want = B / fam.c
        assert M.same_bits(dev.x, want).all(), (what, "x is not b / 2^e")
        if solver in ("pcgn", "pcgn_lambdas"):
            X = dev.x.reshape(fam.F, -1)
            k = X.shape[1]
            assert k == 1 or (M.same_bits(X[:, k // 2], np.zeros(fam.F)).all() and not kw["b"].reshape(fam.F, k)[:, k // 2].any()), (what, "the zero column")


def test_the_strict_solves_freeze_at_different_iterations():
    """the solves of solve_strict on the general system: caps of at most 12 that some column / shift meets while another is done
    before; fs_cg within about 20 iterations"""
    ps = LC.pair_system("general")
    for solver, what, kw in LC.strict_cases(ps):
        kw = dict(kw)
        r = LC.solve_model(ps, solver, lam=ps.s.lam, **kw)
        if solver == "cg":
            assert 2 <= r.iters[0] <= 20 and r.state["done"] == 1.0, (what, r.iters)
        else:
            assert 0 < kw["max_iter"] <= 12 and max(r.iters) <= kw["max_iter"], (what, r.iters)
        if solver == "mscg" or "ladder of 8" in what or "jacobi" in what and solver in ("pcgn", "pcgn_lambdas"):
            assert len(set(r.iters)) >= 3, (what, r.iters)
            if solver in ("pcgn", "pcgn_lambdas"):
                assert r.infos[3].iterations == 0 and r.infos[3].converged == 1, "a column that is done before the first product"


def test_the_solver_operations_reach_everything(sets, gpu_walks):
    """over the walks the GPU test runs, per data set: every solver operation, every solver, solves refused with each status the
    header names and solves that went through on a released pair, the poison before about half of the solves"""
    for name in sets:
        ops, solves, status, poisoned, total = {}, {}, {}, 0, 0
        for w in gpu_walks:
            if w.data.name != name:
                continue
            for k, v in w.counts["ops"].items():
                ops[k] = ops.get(k, 0) + v
            for k, v in w.counts["solves"].items():
                solves[k] = solves.get(k, 0) + v
            for k, v in w.counts["solver_status"].items():
                status[k] = status.get(k, 0) + v
            poisoned += w.counts["poisoned"]
            total += sum(w.counts["solves"].values())
            assert w.counts["poison_seen"] == w.counts["poisoned"]            # (the stand-in's probe sees its one double)
        missing = [o for o in LC.SOLVER_OPS if ops.get(o, 0) < 5]
        assert not missing, (name, missing, ops)
        assert all(solves.get(sv, 0) >= 5 for sv in ("cg", "cg2", "pcg", "mscg", "pcgn", "pcgn_lambdas", "mscgn")), (name, solves)
        for sv in ("gram_diag", "pcg", "pcgn"):
            assert status.get((sv, LC.FS_ERR_RELEASED), 0) >= 1 and status.get((sv, LC.FS_OK), 0) >= 5, (name, sv, status)
        for sv in ("pcgn_lambdas", "mscgn"):                # (the solves of solve_strict and solve_bad_arg count under their solver)
            assert status.get((sv, LC.FS_OK), 0) >= 10, (name, sv, status)
            assert status.get((sv, LC.FS_ERR_RELEASED), 0) >= 1 and status.get((sv, LC.FS_ERR_ARG), 0) >= 1, (name, sv, status)
        assert sum(v for (sv, rc), v in status.items() if rc == LC.FS_ERR_ARG) >= 5, (name, status)
        assert total // 4 <= poisoned <= 3 * total // 4, (name, poisoned, total)


@pytest.mark.parametrize("F,nrow,k,m", [(2000, 6000, 5, 8), (257, 517, 17, 3)])
def test_work_space_is_the_headers_formulas(F, nrow, k, m):
    """LC.work_space -- what poison_heap fills -- against include/fastsparse_hip.h, "Work space per solve": a size that is off makes
    the poison miss silently.  Besides the header's terms every solve has three small blocks (the partial sums 3 kRedBlocks, the 4
    sums, st[]) and fs_mscg its per-shift scalars; a direction (panel) is rounded up to an even count of doubles"""
    import _mscg_model as S
    import _pcgn_model as N
    import os
    text = " ".join(open(os.path.join(M.ROOT, "include", "fastsparse_hip.h")).read().split())
    for words in ("Work space per solve: 3 F + N doubles and one direction of F per shift with sigma != 0",
                  "Work space per solve: 3 k F + k N doubles, F more with a preconditioner, 2048 k for the * partial sums and 512 for the per-column scalars",
                  "Work space per solve: 3 k F + k N doubles (R, P, Q, T), one F x k direction panel per shift with sigma != 0, 2048 k doubles for * the partial sums and 9344 for the scalars",
                  "Work space with the option: 3 w1 F + w2 F doubles more", "and 512 doubles for the scalars in original numbering"):
        assert words in text, words
    fixed = 3 * M.RED_BLOCKS + 4 + M.CG_STATE_DOUBLES
    even = lambda n: (n + 1) & ~1
    nslots = m - 1
    total = lambda *a, **kw: sum(LC.work_space(*a, **kw))
    assert total("cg", F, nrow) == 3 * F + nrow + fixed
    assert total("cg2", F, nrow, 2) == 2 * (3 * F + nrow) + fixed
    assert total("pcg", F, nrow) == 3 * F + nrow + fixed and total("pcg", F, nrow, 1, True) == 4 * F + nrow + fixed
    assert total("mscg", F, nrow, 1, False, nslots) == 3 * F + nrow + even(F) * nslots + S.MAX_SHIFTS * S.MS_STRIDE + fixed
    for solver in ("pcgn", "pcgn_lambdas"):
        assert total(solver, F, nrow, k) == 3 * k * F + k * nrow + 2048 * k + 512 + fixed
        assert total(solver, F, nrow, k, True) == 3 * k * F + k * nrow + F + 2048 * k + 512 + fixed
        w1, w2 = [w for w in (16, 8, 4, 2, 1) if w < k][:2]
        assert total(solver, F, nrow, k, True, widths=(w1, w2)) == 3 * k * F + k * nrow + F + 2048 * k + 512 + fixed + 3 * w1 * F + w2 * F + 512
    assert total("mscgn", F, nrow, k, False, nslots) == 3 * k * F + k * nrow + even(F * k) * nslots + 2048 * k + 9344 + fixed
    assert N.MAX_RHS * N.PN_STRIDE == 512 and 2 * M.RED_BLOCKS == 2048 and LC.MSCGN_SCALARS == 9344
    # one entry per allocation: the blocks the solvers carve up themselves are one size each
    assert 2048 * k + 512 in LC.work_space("pcgn_lambdas", F, nrow, k) and 2048 * k + 9344 in LC.work_space("mscgn", F, nrow, k, False, nslots)
    assert even(F * k) * nslots in LC.work_space("mscgn", F, nrow, k, False, nslots)


@pytest.mark.parametrize("kind", ("exact", "general"))
def test_the_repacking_cases_repack(kind):
    """the solves tests/test_gpu_lifecycle.py runs under option "pcgn_compact" on poisoned work space really narrow: by the models'
    counts the plan holds a segment narrower than k -- and, over the cases, panels with padding columns and more than one repack"""
    ps = LC.pair_system(kind)
    picks = LC.repacking_cases(ps)
    assert len(picks) >= (14 if kind == "exact" else 2) and {sv for sv, _, _ in picks} == set(LC.NARROWING), picks
    padded = repacks = 0
    for solver, i, what in picks:
        cases = LC.strict_cases(ps) if kind == "general" else [c for c in LC.exact_cases(ps.fam) if c[0] == solver]
        sv, name, kw = cases[i]
        assert (sv, name) == (solver, what)
        r = LC.solve_model(ps, solver, **dict(dict(lam=ps.s.lam, tol=ps.s.tol), **kw))
        k = len(r.iters)
        segs = LC.PM.plan(k, [w for w in LC.PM.RUNGS if w < k], r.iters, ["rsq" not in st for st in r.extra], kw.get("max_iter") or ps.s.ncol)
        assert any(w < k for _, w, _ in segs), (what, r.iters, segs)
        padded += any(w > bin(mask).count("1") for _, w, mask in segs)
        repacks += len(segs) > 1
    assert padded >= 1 and (kind == "exact" or repacks >= 2), (kind, padded, repacks)
