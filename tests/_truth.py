"""The mathematical answer for every CG solver after fs_cg2, and the checker that holds a solve against it (helper; no test in here).

Nothing here imports a _*_model.py: the models restate the header's text line by line, as the kernels do, so a recurrence that is
wrong in all three passes every bit-for-bit test.  What stands here instead:

  dense_truth   K = A'A from the COO arrays in numpy.longdouble, ONE eigh of K in float64 (x*(lambda) = V (Lambda + lambda)^-1 V' b
                for every lambda and column at once), then iterative refinement with longdouble residuals until the relative
                residual of x* is below 1e-17 -- asserted.  Relative to ||K + lambda|| ||x|| + ||b||, the normwise backward error:
                relative to ||b|| alone longdouble (eps 1.1e-19) stalls at 3.5e-17 where f = 1e-3 makes ||K|| ||x|| 300 ||b||.
  textbook_pcg  the header's fs_pcg text on dense arrays with plain sums: once in longdouble, and twice in float64 (serial sums,
                numpy's pairwise sums).  The three counts together are "the reference counts" of a column or pair.  A shift
                lambda_i of a multi-shift solve is one independent CG at lambda_i: in exact arithmetic multi-shift CG's x_i after n
                iterations is that CG's iterate.
  make_case     one random draw: the matrix, lambdas, right-hand sides, preconditioner, start, caps, tolerances, layout and options.
  check         one solve of one solver (X, the infos, the status, the buffers around X and B) against all of the above.  It knows
                nothing about where the solve came from: the device (tests/_fuzz_solvers.py) and the CPU models
                (tests/test_truth_reference.py) go through the same code.

The count class.  A column is IN THE COUNT CLASS when lambda = f max(1, mean Gram diagonal) has f >= 1 and the matrix is not a
`scaled` one solved without a preconditioner (fs_mscg / fs_mscgn have none: `scaled` is never in their class).  On the class the
reference alone always converged within F iterations and its three counts differed by at most 1 (400 draws of seed 20261022 on
the CPU: 2773 pairs, 19 of them one apart, none more); with f = 1e-3 they differ by up to 15 and some solves do not finish in F.  No count and no capped iterate is compared outside the
class.  make_case draws f and the matrix kind so that at least 60 % of every solver's cases are in the class (the runs assert it).

The bar of check 5 (a capped x against the longdouble iterate of the same number): the float64 textbook loops against the longdouble
one over the seeded stretch of tests/test_gpu_fuzz_solvers.py, the worst relative deviation in the 2-norm: 2.5e-13 (CAPPED_MEASURED;
draw 36, one row of 28 entries under a caller's diagonal, after five iterations; 1.7e-12 over 300 draws of another seed).  Times 100,
because the device adds in a two-stage tree that neither textbook loop uses: 2.5e-11 (CAPPED_BAR).

Where make_case departs from a free draw, and why:
  nrow = 20000 is not drawn with 25 entries per row (K in longdouble costs the sum of the squared row lengths);
  tol = 0 (with a cap) is drawn only for F >= 63 and nrow >= 300, where K + lambda has far more distinct eigenvalues than the cap has
  iterations: a solve of F <= 3 unknowns, or on a K of rank 1, is finished within the cap and reaches r = 0 exactly; the next alpha
  is 0 / 0 -- a NaN column, which no case is to have.  Nor is it drawn with a start that holds x* rounded to double (warm_exact,
  mixed): such a solve iterates on rounding noise, and "no further from x* than the start" (check 5) is a property of exact
  arithmetic that no float64 loop keeps at the rounding floor (the models end at 1.4e-47 from 7.9e-48 on such a draw)."""
import collections

import numpy as np

LD = np.longdouble
FS_OK = 0
NONE, JACOBI, DIAG = 0, 1, 2
SOLVERS = ("pcg", "mscg", "pcgn", "pcgn_lambdas", "mscgn", "dist_pcg", "dist_pcgn", "dist_pcgn_lambdas", "dist_mscg", "dist_mscgn")
MODES = ("default", "reproducible", "strict_order", "cg_fixed_order=0", "spmv_kernel")
STARTS = ("cold", "warm_random", "warm_exact", "mixed")
GUARD = 4                                                           # doubles in front of and behind X and B (even: keeps alignment)
FILL = np.int64(0x7FF80BADF00D0001)                                 # what guards, gaps and a cold X are filled with (a NaN)
TEXTBOOK_PAIRS = 16
CLASS_FLOOR = 0.6
CAPPED_MEASURED = 2.5e-13                                           # (re-measured by test_truth_reference.py: must not be exceeded)
CAPPED_BAR = 100 * CAPPED_MEASURED

Result = collections.namedtuple("Result", "solver cap tol status xbuf bbuf infos again")   # again: (xbuf, infos) of a second run or None
Info = collections.namedtuple("Info", "iterations converged rnorm bnorm")
Ref = collections.namedtuple("Ref", "iterations converged rnorm bnorm x")


class CheckFailed(AssertionError):
    """a solve missed a check: .name says which ("status", "true residual", "info", "iteration count", "energy norm",
    "capped iterate", "frozen", "twins", "repeat")"""

    def __init__(self, name, detail):
        super().__init__(f"{name}: {detail}")
        self.name = name


def family(solver):
    return solver[5:] if solver.startswith("dist_") else solver


def preconditioned(solver):
    return family(solver) in ("pcg", "pcgn", "pcgn_lambdas")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _norm(v):
    return np.sqrt((v * v).sum(0))


# ---- the draw --------------------------------------------------------------------------------------------------------------
def _pick(rng, values, p=None):
    return values[int(rng.choice(len(values), p=None if p is None else np.asarray(p, float) / np.sum(p)))]


class Case:
    """one draw of make_case; everything a backend needs to run it and check() needs to judge it"""

    def __repr__(self):
        return (f"case(seed={self.seed}, draw={self.draw}: {self.nrow}x{self.F} {self.kind} nnz={self.rows.size} f={self.f:g} k={self.k} "
                f"m={self.m} precond={self.precond} start={self.start} cap={self.cap} tol={self.tol:g}/{self.tol_cap:g} mode={self.mode} "
                f"pcgn_kernel={self.pcgn_kernel} compact={self.pcgn_compact} ranks={self.ranks} scheme={self.scheme} "
                f"gap={self.ldx_gap} misalign={self.misalign} device_t={self.device_t})")

    # -- shapes and lambdas per solver
    def shape(self, solver):
        """(m, k) of the solver's X: m panels of F x k"""
        fam = family(solver)
        return (self.m if fam in ("mscg", "mscgn") else 1, 1 if fam in ("pcg", "mscg") else self.k)

    def lams(self, solver):
        """lambda of pair (i, j) as an (m, k) array"""
        m, k = self.shape(solver)
        fam = family(solver)
        if fam in ("mscg", "mscgn"):
            return np.repeat(np.asarray(self.ladder)[:, None], k, 1)
        if fam == "pcgn_lambdas":
            return np.asarray(self.lams_k)[None, :].copy()
        return np.full((1, k), self.lam)

    def B_of(self, solver):
        return np.ascontiguousarray(self.B[:, :self.shape(solver)[1]])

    def in_class(self, solver):
        with_precond = preconditioned(solver) and self.precond != NONE
        return self.f >= 1 and not (self.kind == "scaled" and not with_precond)

    def warm(self, solver):
        return preconditioned(solver) and self.start != "cold"

    def start_of(self, solver, j):
        """how column j starts: "cold", "warm_random", "warm_exact" ("mixed": the columns take turns)"""
        if not self.warm(solver):
            return "cold"
        return self.start if self.start != "mixed" else ("warm_exact", "warm_random", "zero")[j % 3]

    def twins(self, solver):
        """(j, twin): column j has the bits of column twin's b (and lambda, and start)"""
        k = self.shape(solver)[1]
        return [(j, t) for j, t in self._twins if j < k and t < k]

    # -- the truth, once per case
    def truth(self):
        if self._truth is None:
            self._truth = dense_truth(self)
        return self._truth

    def X0(self, solver):
        """(F, k) warm start of a preconditioned solver, or None"""
        if not self.warm(solver):
            return None
        if solver not in self._x0:
            k = self.shape(solver)[1]
            lams = self.lams(solver)[0]
            xs = self.truth().xstar(lams, np.arange(k))                        # (F, k) longdouble
            X0 = np.zeros((self.F, k))
            for j in range(k):
                how = self.start_of(solver, j)
                if how == "warm_exact":
                    X0[:, j] = xs[:, j].astype(np.float64)
                elif how == "warm_random":
                    X0[:, j] = self.x0_noise[:, j] * float(np.sqrt((xs[:, j] * xs[:, j]).sum()) / np.sqrt(self.F))
            for j, t in self.twins(solver):
                X0[:, j] = X0[:, t]
            X0[:, ~self.B_of(solver).any(0)] = 0.0
            self._x0[solver] = X0
        return self._x0[solver]

    def diag_of(self, solver):
        return self.diag if preconditioned(solver) and self.precond == DIAG else None

    # -- the buffers a backend hands to the solver
    def layout(self, solver):
        """(offset of X, ldx, doubles of X's buffer, offset of B, doubles of B's buffer)"""
        m, k = self.shape(solver)
        ne = self.F * k
        off = GUARD + (1 if self.misalign else 0)
        ldx = ne + (3 if self.ldx_gap else 0)
        return off, ldx, off + (m - 1) * ldx + ne + GUARD, off, off + ne + GUARD

    def buffers(self, solver):
        """X's and B's buffers as host arrays: guards, gaps and a cold X hold FILL, a warm X holds X0"""
        m, k = self.shape(solver)
        xoff, ldx, nx, boff, nb = self.layout(solver)
        ne = self.F * k
        xbuf = np.full(nx, FILL, np.int64).view(np.float64)
        bbuf = np.full(nb, FILL, np.int64).view(np.float64)
        bbuf[boff:boff + ne] = self.B_of(solver).reshape(-1)
        X0 = self.X0(solver)
        if X0 is not None:
            xbuf[xoff:xoff + ne] = X0.reshape(-1)
        return xbuf, bbuf

    def X_of(self, solver, xbuf):
        """(m, F, k) out of X's buffer"""
        m, k = self.shape(solver)
        xoff, ldx, _, _, _ = self.layout(solver)
        ne = self.F * k
        return np.stack([xbuf[xoff + i * ldx:xoff + i * ldx + ne].reshape(self.F, k) for i in range(m)])

    def solves(self):
        """(cap, tol) of the two solves of a case: run to F, and capped"""
        return ((0, self.tol), (self.cap, self.tol_cap))


def make_case(rng, seed=0, draw=0):
    c = Case()
    c.seed, c.draw, c._truth, c._x0, c._refs = seed, draw, None, {}, {}
    c.F = F = int(_pick(rng, (1, 2, 3, 63, 64, 65, 255, 256, 257, 513), (1, 1, 1, 2, 2, 2, 1, 1, 1, 1)))
    c.nrow = nrow = int(_pick(rng, (1, 50, 300, 3000, 20000), (1, 2, 3, 2, 1)))
    mean = float(_pick(rng, (1.5, 6.0, 25.0)))
    if nrow == 20000 and mean == 25.0:
        mean = 6.0
    lens = rng.poisson(mean, nrow)
    lens[0] = max(lens[0], 1)                                                  # (no matrix without an entry)
    rows = np.repeat(np.arange(nrow, dtype=np.int32), lens)
    cols = rng.integers(0, F, rows.size).astype(np.int32)
    order = rng.permutation(rows.size)
    c.rows, c.cols = np.ascontiguousarray(rows[order]), np.ascontiguousarray(cols[order])
    c.kind = _pick(rng, ("binary", "valued", "scaled"), (0.45, 0.40, 0.15))
    c.vals = None
    if c.kind != "binary":
        c.vals = rng.standard_normal(rows.size)
        if c.kind == "scaled":
            c.vals = c.vals * (10.0 ** rng.uniform(-2, 2, F))[c.cols]
        c.vals = np.ascontiguousarray(c.vals)
    gram = np.bincount(c.cols, weights=None if c.vals is None else c.vals * c.vals, minlength=F).astype(np.float64)
    c.f = float(_pick(rng, (1e-3, 1.0, 30.0), (0.15, 0.45, 0.40)))
    c.lam = c.f * max(1.0, float(gram.mean()))
    ks, ms = (1, 2, 3, 4, 5, 8, 16, 17, 32), (1, 3, 8, 16)
    c.k = int(_pick(rng, ks, (3, 2, 2, 2, 2, 2, 1, 1, 1))) if rng.uniform() < 0.8 else int(rng.integers(1, 33))
    c.m = int(_pick(rng, ms, (2, 3, 2, 1))) if rng.uniform() < 0.8 else int(rng.integers(1, 17))

    def ladder(n):
        """geometric above lam, shuffled, some rungs twice"""
        top = 10.0 ** rng.uniform(0.5, 7.0)
        v = c.lam * top ** (np.arange(n) / max(n - 1, 1))
        for _ in range(int(rng.integers(0, 3))):
            if n >= 2:
                a, b = rng.integers(0, n, 2)
                v[a] = v[b]
        return [float(x) for x in rng.permutation(v)]

    c.ladder, c.lams_k = ladder(c.m), ladder(c.k)
    B = rng.standard_normal((F, c.k)) * np.ldexp(1.0, rng.integers(-100, 101, c.k))[None, :]
    c._twins = []
    special = rng.uniform()
    if special < 0.15:
        B[:] = B[:, :1]                                                        # the same b in every column
    if c.k >= 2 and rng.uniform() < 0.4:
        j, t = (int(v) for v in rng.permutation(c.k)[:2])
        B[:, j] = B[:, t]
        c.lams_k[j] = c.lams_k[t]
        c._twins.append((j, t))
    if rng.uniform() < (0.35 if c.k >= 2 else 0.1):
        z = int(rng.integers(0, c.k))
        if all(z not in tw for tw in c._twins):
            B[:, z] = 0.0
    c.B = np.ascontiguousarray(B)
    c.precond = int(_pick(rng, (NONE, JACOBI, DIAG), (1, 2, 1)))
    c.diag = (gram + c.lam) * (1.0 + 0.5 * np.cos(np.arange(F) * 1.7)) + 0.125
    c.start = _pick(rng, STARTS)
    c.x0_noise = rng.standard_normal((F, c.k))
    c.cap = int(rng.integers(1, 6))
    c.tol = float(_pick(rng, (1e-6, 1e-10)))
    c.tol_cap = 0.0 if F >= 63 and nrow >= 300 and c.start in ("cold", "warm_random") and rng.uniform() < 0.4 else c.tol
    c.ldx_gap, c.misalign = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    c.mode = _pick(rng, MODES, (3, 2, 2, 2, 1))
    c.pcgn_kernel, c.pcgn_compact = int(rng.integers(0, 3)), int(rng.integers(0, 2))
    c.ranks, c.scheme, c.device_t = int(_pick(rng, (1, 3, 5))), int(rng.integers(0, 2)), bool(rng.integers(0, 2))
    return c


def stretch(seed, n):
    """the n cases of a seeded stretch, each from a generator of its own (so that --cases replays one draw without the others)"""
    return [make_case(np.random.default_rng([seed, d]), seed, d) for d in range(n)]


# ---- the dense truth -------------------------------------------------------------------------------------------------------
def gram_longdouble(nrow, F, rows, cols, vals):
    """K = A'A in longdouble from COO (duplicates add): row by row, the outer product of the row's entries"""
    K = np.zeros((F, F), LD)
    if rows.size == 0:
        return K
    order = np.argsort(rows, kind="stable")
    r, cc = rows[order], cols[order].astype(np.int64)
    v = np.ones(r.size, LD) if vals is None else vals[order].astype(LD)
    start = np.flatnonzero(np.concatenate(([True], r[1:] != r[:-1])))
    lens = np.diff(np.concatenate((start, [r.size])))
    for n in np.unique(lens):
        at = start[lens == n][:, None] + np.arange(n)[None, :]                 # (rows of this length, n)
        ci, vi = cc[at], v[at]
        flat = (ci[:, :, None] * F + ci[:, None, :]).reshape(-1)
        np.add.at(K.reshape(-1), flat, (vi[:, :, None] * vi[:, None, :]).reshape(-1))
    return K


class Truth:
    def __init__(self, K):
        self.K = K
        self.K64 = K.astype(np.float64)
        self.w, self.V = np.linalg.eigh(self.K64)
        self.normK = np.sqrt((K * K).sum())
        self._x = {}
        self.B = None

    def _solve64(self, lam, R):
        return self.V @ ((self.V.T @ R) / (self.w + lam)[:, None])

    def xstar(self, lams, cols):
        """x*(lams[n]) for column cols[n] of the case's B: (F, len) longdouble, refined until
        ||b - (K + lam) x|| <= 1e-17 (||K + lam|| ||x|| + ||b||)"""
        lams, cols = [float(v) for v in lams], [int(j) for j in cols]
        todo = sorted({(lam, j) for lam, j in zip(lams, cols) if (lam, j) not in self._x})
        for lam in sorted({lam for lam, _ in todo}):
            js = [j for l2, j in todo if l2 == lam]
            Bj = self.B[:, js].astype(LD)
            norm = np.sqrt((Bj * Bj).sum(0))
            X = self._solve64(lam, self.B[:, js]).astype(LD)
            for _ in range(12):
                R = Bj - (self.K @ X + LD(lam) * X)
                rel = np.sqrt((R * R).sum(0)) / np.where(norm == 0, LD(1), (self.normK + LD(lam)) * np.sqrt((X * X).sum(0)) + norm)
                if (rel <= LD(1e-17)).all():
                    break
                X = X + self._solve64(lam, R.astype(np.float64)).astype(LD)
            assert (rel <= LD(1e-17)).all(), ("dense_truth: refinement stalled", lam, [float(v) for v in rel])
            for n, j in enumerate(js):
                self._x[(lam, j)] = X[:, n]
        return np.stack([self._x[(lam, j)] for lam, j in zip(lams, cols)], 1)


def dense_truth(case):
    t = Truth(gram_longdouble(case.nrow, case.F, case.rows, case.cols, case.vals))
    t.B = case.B
    # fs_gram_diag as the header defines it: the sum of v^2 over the ENTRIES of a column.  Where (row, column) pairs repeat this is not
    # the diagonal of K (v1^2 + v2^2 against (v1 + v2)^2); Jacobi's M is then another diagonal, and the solve's answer the same
    t.gram = np.zeros(case.F, LD)
    np.add.at(t.gram, case.cols, LD(1) if case.vals is None else case.vals.astype(LD) ** 2)
    return t


# ---- the textbook loop -----------------------------------------------------------------------------------------------------
def _sums(how):
    """(sum of a vector, row sums of a matrix) in the dtype of the data"""
    if how == "serial":
        return (lambda v: np.add.accumulate(v)[-1] if v.size else v.dtype.type(0),
                lambda Mx: np.add.accumulate(Mx, axis=1)[:, -1] if Mx.shape[1] else np.zeros(Mx.shape[0], Mx.dtype))
    return (lambda v: v.sum(), lambda Mx: Mx.sum(axis=1))


def textbook_loop(K, b, lam, tol, max_iter, d=None, x0=None, dtype=LD, how="plain", updates=None):
    """the header's fs_pcg text on a dense K = A'A (so t = A p, q = A' t is q = K p): x, count, converged, rnorm, bnorm as fs_pcg_info
    has them.  d: the preconditioner's diagonal or None.  updates: ignore the stopping rule and return x after exactly that many
    updates of x (the iterate a capped or stopped solve is compared with)."""
    T = dtype
    dot, rowsum = _sums(how)
    K, b, lam, tol = K.astype(T), np.asarray(b).astype(T), T(lam), T(tol)
    F = b.size
    cap = max_iter if max_iter > 0 else F
    with np.errstate(all="ignore"):
        dinv = None if d is None else np.where(np.asarray(d).astype(T) == 0, T(1), T(1) / np.asarray(d).astype(T))
        if x0 is None:
            x, r = np.zeros(F, T), b.copy()
        else:
            x = np.asarray(x0).astype(T)
            q = rowsum(K * x[None, :])
            q = q + lam * x
            r = b - q
        bb, rr = dot(b * b), dot(r * r)
        stop = tol * np.sqrt(bb)
        if updates is None and np.sqrt(rr) <= stop:
            return Ref(0, 1, np.sqrt(rr), np.sqrt(bb), x)
        if updates == 0:
            return Ref(0, 0, np.sqrt(rr), np.sqrt(bb), x)
        z = r if dinv is None else r * dinv
        p = z.copy()
        rz = dot(r * z)
        count, converged = 0, 0
        for n in range(cap if updates is None else updates):
            q = rowsum(K * p[None, :])
            q = q + lam * p
            alpha = rz / dot(q * p)
            x = x + alpha * p
            r = r - alpha * q
            rr = dot(r * r)
            if updates is None and np.sqrt(rr) <= stop:
                converged = 1
                break
            z = r if dinv is None else r * dinv
            rzn = dot(r * z)
            beta = rzn / rz
            rz = rzn
            count += 1
            p = z + beta * p
    return Ref(count, converged, np.sqrt(rr), np.sqrt(bb), x)


def textbook_pcg(K, b, lam, tol, max_iter, d=None, x0=None):
    """the longdouble run and the two float64 runs (serial sums, numpy's pairwise sums) of one column or pair"""
    return (textbook_loop(K, b, lam, tol, max_iter, d, x0, LD, "plain"),
            textbook_loop(K, b, lam, tol, max_iter, d, x0, np.float64, "serial"),
            textbook_loop(K, b, lam, tol, max_iter, d, x0, np.float64, "plain"))


def precond_diag(case, solver, truth, lam):
    """the diagonal the solver's preconditioner holds for a column at lam, or None"""
    if not preconditioned(solver) or case.precond == NONE:
        return None
    return case.diag if case.precond == DIAG else (truth.gram + LD(lam))


def textbook_pairs(case, solver):
    """the pairs (i, j) the textbook loop runs on: all when m k <= 16, else 16 with the first and last column and the smallest and
    largest lambda among them"""
    m, k = case.shape(solver)
    pairs = [(i, j) for i in range(m) for j in range(k)]
    if len(pairs) <= TEXTBOOK_PAIRS:
        return pairs
    lams = case.lams(solver)
    lo, hi = np.unravel_index(np.argmin(lams), lams.shape), np.unravel_index(np.argmax(lams), lams.shape)
    must = [(0, 0), (m - 1, k - 1), (int(lo[0]), int(lo[1])), (int(hi[0]), int(hi[1])), (int(lo[0]), 0), (int(hi[0]), k - 1)]
    keep = list(dict.fromkeys(must))
    rest = [p for p in pairs if p not in keep]
    order = np.random.default_rng([case.seed, case.draw, 7]).permutation(len(rest))
    return keep + [rest[n] for n in order[:TEXTBOOK_PAIRS - len(keep)]]


def reference(case, solver, cap, tol, i, j):
    """the three textbook runs of pair (i, j) of a solve, once per case"""
    key = (family(solver), cap, tol, i, j)
    if key not in case._refs:
        t = case.truth()
        lam = float(case.lams(solver)[i, j])
        X0 = case.X0(solver)
        case._refs[key] = textbook_pcg(t.K, case.B[:, j], lam, tol, cap, precond_diag(case, solver, t, lam), None if X0 is None else X0[:, j])
    return case._refs[key]


def measure_capped(cases):
    """the worst relative deviation (2-norm) of a float64 textbook loop from the longdouble one at the capped iterate, over the
    textbook pairs of the count class of `cases`, where the three loops took the same number of updates"""
    worst = 0.0
    for case in cases:
        for solver in ("pcgn", "pcgn_lambdas", "mscgn"):
            if not case.in_class(solver):
                continue
            for i, j in textbook_pairs(case, solver):
                ld, serial, pairwise = reference(case, solver, case.cap, case.tol_cap, i, j)
                scale = _norm(ld.x)
                for other in (serial, pairwise):
                    if (other.iterations, other.converged) == (ld.iterations, ld.converged) and scale != 0:
                        worst = max(worst, float(_norm(other.x.astype(LD) - ld.x) / scale))
    return worst


# ---- the checker -----------------------------------------------------------------------------------------------------------
def check(case, result):
    """hold one solve against the truth; raises CheckFailed named after the first check that fails.  Returns what the summary
    lines count: {"class": in the count class, "counts": [(count, min ref, max ref)], "at_cap": pairs that ended at the cap}."""
    solver, cap, tol = result.solver, result.cap, result.tol
    m, k = case.shape(solver)
    F = case.F
    what = (repr(case), solver, f"cap={cap} tol={tol:g}")

    def fail(name, *detail):
        raise CheckFailed(name, (what,) + detail)

    # 1. status, finiteness, the doubles around X and B
    if result.status != FS_OK:
        fail("status", result.status)
    xoff, ldx, nx, boff, nb = case.layout(solver)
    ne = F * k
    xbuf0, bbuf0 = case.buffers(solver)
    if result.xbuf.size != nx or result.bbuf.size != nb:
        fail("status", "buffer sizes", result.xbuf.size, nx, result.bbuf.size, nb)
    if not np.array_equal(_bits(result.bbuf), _bits(bbuf0)):
        fail("status", "B or a guard double around it was written")
    outside = np.ones(nx, bool)
    for i in range(m):
        outside[xoff + i * ldx:xoff + i * ldx + ne] = False
    if not (_bits(result.xbuf)[outside] == FILL).all():
        fail("status", "a guard double around X or a gap between its panels was written", np.flatnonzero(outside & (_bits(result.xbuf) != FILL))[:4])
    X = case.X_of(solver, result.xbuf)
    if not np.isfinite(X).all():
        fail("status", "X is not finite")
    infos = [[result.infos[i * k + j] for j in range(k)] for i in range(m)]
    lams = case.lams(solver)
    truth = case.truth()
    B = case.B_of(solver)
    Bl = B.astype(LD)
    bnorm = _norm(Bl)
    limit = cap if cap > 0 else F

    # residuals of every pair in longdouble: R = B - (K + lam) X
    Xl = X.astype(LD)
    R = np.stack([Bl - (truth.K @ Xl[i] + lams[i].astype(LD)[None, :] * Xl[i]) for i in range(m)])
    rnorm = np.stack([_norm(R[i]) for i in range(m)])

    # 2. the true residual of a converged pair
    for i in range(m):
        for j in range(k):
            if infos[i][j].converged == 1 and not rnorm[i, j] <= LD(2.0 * tol) * bnorm[j]:
                fail("true residual", (i, j), float(rnorm[i, j]), float(bnorm[j]), "tol", tol)

    # 3. the info fields
    in_class = case.in_class(solver)
    for i in range(m):
        for j in range(k):
            g = infos[i][j]
            if not abs(LD(g.bnorm) - bnorm[j]) <= LD(1e-13) * bnorm[j]:
                fail("info", (i, j), "bnorm", g.bnorm, float(bnorm[j]))
            if g.converged != int(g.rnorm <= np.float64(tol) * np.float64(g.bnorm)):
                fail("info", (i, j), "converged", g.converged, g.rnorm, tol * g.bnorm)
            if not 0 <= g.iterations <= limit:
                fail("info", (i, j), "iterations beyond the cap", g.iterations, limit)
            if g.converged != 1 and g.iterations != limit:
                fail("info", (i, j), "not converged before the cap", g.iterations, limit)
            if in_class and cap == 0 and g.converged != 1:
                fail("info", (i, j), "a column of the count class did not converge within F")

    # 4. the counts against the textbook loops, on the count class
    counts = []
    if in_class:
        for i, j in textbook_pairs(case, solver):
            g = infos[i][j]
            refs = reference(case, solver, cap, tol, i, j)
            lo, hi = min(r.iterations for r in refs), max(r.iterations for r in refs)
            counts.append((g.iterations, lo, hi))
            if not lo - 1 <= g.iterations <= hi + 1:
                fail("iteration count", (i, j), g.iterations, [r.iterations for r in refs])

    # 5a. CG minimises the error in the K + lam norm: no solve ends further from x* than it started
    if cap > 0:
        X0 = case.X0(solver)
        for i in range(m):
            xs = truth.xstar(lams[i], np.arange(k))
            e2 = ((xs - Xl[i]) * R[i]).sum(0)                                  # (x* - x)' (K + lam) (x* - x): (K + lam)(x* - x) = R
            if X0 is None:
                e0 = (xs * Bl).sum(0)
            else:
                X0l = X0.astype(LD)
                R0 = Bl - (truth.K @ X0l + lams[i].astype(LD)[None, :] * X0l)
                e0 = ((xs - X0l) * R0).sum(0)
            bad = ~(np.sqrt(np.maximum(e2, 0)) <= np.sqrt(np.maximum(e0, 0)) * LD(1 + 1e-10))
            if bad.any():
                j = int(np.flatnonzero(bad)[0])
                fail("energy norm", (i, j), float(np.sqrt(max(e2[j], 0))), float(np.sqrt(max(e0[j], 0))))

    # 5b. a capped x of the count class against the longdouble iterate of the same number
    if cap > 0 and in_class:
        for i, j in textbook_pairs(case, solver):
            g = infos[i][j]
            if bnorm[j] != 0:
                lam = float(lams[i, j])
                X0 = case.X0(solver)
                # a converged pair with count n took n + 1 updates -- or none, when count 0 means frozen at the start
                tries = [g.iterations] if g.converged != 1 else ([0, 1] if g.iterations == 0 else [g.iterations + 1])
                devs = []
                for updates in tries:
                    want = textbook_loop(truth.K, case.B[:, j], lam, tol, cap, precond_diag(case, solver, truth, lam),
                                         None if X0 is None else X0[:, j], LD, "plain", updates=min(updates, limit)).x
                    scale = _norm(want)
                    devs.append(LD(0) if scale == 0 and not Xl[i][:, j].any() else (_norm(Xl[i][:, j] - want) / scale if scale != 0 else LD(np.inf)))
                if not min(devs) <= LD(CAPPED_BAR):
                    fail("capped iterate", (i, j), float(min(devs)), CAPPED_BAR, "updates", tries)

    # 6. frozen from the start
    X0 = case.X0(solver)
    for j in range(k):
        if bnorm[j] == 0:
            for i in range(m):
                g = infos[i][j]
                if not ((_bits(X[i][:, j]) == 0).all() and g.iterations == 0 and g.converged == 1):
                    fail("frozen", (i, j), "a zero column is not +0.0 with count 0", g.iterations, g.converged)
        elif X0 is not None and case.start_of(solver, j) == "warm_exact" and tol > 0:
            x0 = X0[:, j].astype(LD)
            r0 = _norm(Bl[:, j] - (truth.K @ x0 + LD(float(lams[0, j])) * x0))
            if r0 <= LD(0.5 * tol) * bnorm[j]:
                g = infos[0][j]
                if not (np.array_equal(_bits(X[0][:, j]), _bits(X0[:, j])) and g.iterations == 0 and g.converged == 1):
                    fail("frozen", (0, j), "a warm start from a converged x did not come back as it was", g.iterations, g.converged)

    # 7. duplicates and repeats
    fixed_order = case.mode != "cg_fixed_order=0"
    if fixed_order:
        for j, t in case.twins(solver):
            for i in range(m):
                if not (np.array_equal(_bits(X[i][:, j]), _bits(X[i][:, t])) and tuple(infos[i][j]) == tuple(infos[i][t])):
                    fail("twins", (i, j, t), "a duplicate column does not have the bits of its twin")
    if fixed_order and result.again is not None:
        xbuf2, infos2 = result.again
        if not np.array_equal(_bits(xbuf2), _bits(result.xbuf)):
            fail("repeat", "the same solve again: X differs", int((_bits(xbuf2) != _bits(result.xbuf)).sum()))
        if [tuple(g) for g in infos2] != [tuple(g) for g in result.infos]:
            fail("repeat", "the same solve again: the infos differ")
    at_cap = sum(1 for i in range(m) for j in range(k) if infos[i][j].converged != 1)
    return {"class": in_class, "counts": counts, "at_cap": at_cap}


# ---- relations the header states: two solves, bit for bit ------------------------------------------------------------------
def same_pair(what, X_a, info_a, X_b, info_b):
    """a column of one solve against a column of another: X and the info, bit for bit"""
    if not (np.array_equal(_bits(X_a), _bits(X_b)) and tuple(info_a) == tuple(info_b)):
        raise CheckFailed("relation", (what, int((_bits(X_a) != _bits(X_b)).sum()), tuple(info_a), tuple(info_b)))


# ---- the summary -----------------------------------------------------------------------------------------------------------
class Tally:
    """what a run reports per solver: cases, the share in the count class, the spread of counts, the solves that ended at a cap"""

    def __init__(self):
        self.cases = self.in_class = self.at_cap = self.solves = 0
        self.lo, self.hi, self.spread = None, None, 0

    def add(self, case, solver, outs):
        self.cases += 1
        self.in_class += int(case.in_class(solver))
        for out in outs:
            self.solves += 1
            self.at_cap += int(out["at_cap"] > 0)
            for got, lo, hi in out["counts"]:
                self.lo = got if self.lo is None else min(self.lo, got)
                self.hi = got if self.hi is None else max(self.hi, got)
                self.spread = max(self.spread, got - lo, hi - got, hi - lo)

    def share(self):
        return self.in_class / max(self.cases, 1)

    def line(self, solver):
        return (f"{solver}: {self.cases} cases, {100 * self.share():.0f} % in the count class, counts {self.lo} .. {self.hi} "
                f"(at most {self.spread} from a reference count), {self.at_cap} of {self.solves} solves ended at a cap")
