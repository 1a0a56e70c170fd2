"""A CPU restatement of the CG solvers' device arithmetic (libfastsparse_amd/csrc/fs_cg.hip), for bit-for-bit tests.

Every operation is one IEEE double operation, rounded once, in the order the kernels perform it: the library is built with
-ffp-contract=off, so no multiply and add are fused (the f64 division and square root expansions are correctly rounded).

Reductions have the fixed launch shape of fs_cg.hip:
  stage 1  kRedBlocks x kRedThreads threads.  Thread (b, t) adds 0.0 + its terms i = b kRedThreads + t, + kRedBlocks kRedThreads,
           ... in increasing i.  Each 64-lane wave folds by __shfl_xor for m = 32 .. 1, which leaves lane 0 the pairwise tree
           v[:32] + v[32:], then [:16] + [16:32], ...  The block sum is (((0.0 + w0) + w1) + w2) + w3 over the block's waves.
  stage 2  one block (final_sum_kernel / final_step_kernel).  Thread t adds 0.0 + part[t] + part[t + kRedThreads] + ... over the
           nblocks partials, then the same block tree.  Three sums (cg2) are three independent trees.
A running sum that starts at +0.0 is never -0.0, so padding a thread's terms with +0.0 changes nothing.

The scalar steps are final_step_kernel's kStepCgStart .. kStepCg2Psi (CgStep, fs_common.h) and solve2sym_dev; the two-column
solve takes its column norms and scale factors on the host (cg2_dev_init).  Products are parameters: the oracle's storage-order
products over the CSR the library holds stand in for the device's strict_order products.  tree="serial" makes every sum one
left-to-right loop, as oracle/fs_oracle_cg.c does; `bounds` (the row cuts of A') gives the "gather" scheme of fs_dist_cg: every
rank reduces its own slice, and the rank values are added by stage 2 with nblocks = number of ranks."""
import collections
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libfastsparse_amd", "csrc")

# the model's copies of the launch shape and the state layout; test_cg_model.py asserts them against the sources
RED_BLOCKS, RED_THREADS, WAVE = 1024, 256, 64
CG_PART_DOUBLES, CG_STATE_DOUBLES = 3 * 1024, 16
# st[] of one right-hand side and of two (enum above final_step_kernel); a tuple names consecutive doubles
ST1 = {"done": 0, "iter": 1, "rsq": 2, "alpha": 3, "beta": 4, "stop": 5}
ST2 = {"done": 0, "iter": 1, "RtR": (2, 3), "Alpha": (5, 4), "Psi": (9, 4), "tolsq": 13}
SOURCE_NAMES = {"kRedBlocks": RED_BLOCKS, "kRedThreads": RED_THREADS, "kCgPartDoubles": CG_PART_DOUBLES,
                "kCgStateDoubles": CG_STATE_DOUBLES, "kStDone": 0, "kStIter": 1, "kStRsq": 2, "kStAlpha": 3, "kStBeta": 4,
                "kStStop": 5, "kSt2RtR": 2, "kSt2Alpha": 5, "kSt2Psi": 9, "kSt2Tolsq": 13, "kStDoubles": CG_STATE_DOUBLES}


def source_constants():
    """the integer constants of fs_cg.hip and fs_common.h (constexpr int and enum members), evaluated"""
    text = ""
    for f in ("fs_common.h", "fs_cg.hip"):
        with open(os.path.join(CSRC, f)) as fh:
            text += fh.read() + "\n"
    decls = re.findall(r"constexpr\s+int\s+([^;]*);", text) + re.findall(r"\benum\s*\{([^}]*)\}", text)
    env = {}
    for decl in decls:
        for item in decl.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*([\w\s*+/()-]+?)\s*", item)
            if m:
                try:
                    env[m.group(1)] = int(eval(m.group(2), {"__builtins__": {}}, dict(env)))
                except NameError:
                    pass
    return env


# ---- reductions ------------------------------------------------------------------------------------------------------
def _wave_tree(v):
    """(..., 64) -> (...): lane 0 after the __shfl_xor butterfly"""
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def _block_sum(v):
    """(..., kRedThreads) thread values -> (...): block_sum of fs_cg.hip"""
    w = _wave_tree(v.reshape(v.shape[:-1] + (RED_THREADS // WAVE, WAVE)))
    s = np.zeros(v.shape[:-1])
    for j in range(RED_THREADS // WAVE):
        s = s + w[..., j]
    return s


def _strided(terms, nthreads):
    """thread t: 0.0 + terms[t] + terms[t + nthreads] + ..."""
    terms = np.asarray(terms, np.float64).reshape(-1)
    rounds = -(-terms.size // nthreads)
    pad = np.zeros(rounds * nthreads)
    pad[:terms.size] = terms
    v = np.zeros(nthreads)
    for k in range(rounds):
        v = v + pad[k * nthreads:(k + 1) * nthreads]
    return v


def stage1(terms):
    """the kRedBlocks partials of a grid-stride kernel's block_sum"""
    return _block_sum(_strided(terms, RED_BLOCKS * RED_THREADS).reshape(RED_BLOCKS, RED_THREADS))


def stage2(part):
    """final_sum_kernel / final_step_kernel over nblocks = len(part) partials"""
    return np.float64(_block_sum(_strided(part, RED_THREADS)))


def serial_sum(terms):
    """0.0 + t0 + t1 + ... left to right (ufunc.accumulate is a sequential loop)"""
    return np.float64(np.add.accumulate(np.concatenate(([0.0], np.asarray(terms, np.float64).reshape(-1))))[-1])


class Reducer:
    def __init__(self, tree="device", bounds=None):
        assert tree in ("device", "serial"), tree
        assert bounds is None or tree == "device"
        self.tree, self.bounds = tree, None if bounds is None else [int(b) for b in bounds]

    def __call__(self, terms):
        if self.tree == "serial":
            return serial_sum(terms)
        if self.bounds is None:
            return stage2(stage1(terms))
        ranks = [stage2(stage1(terms[lo:hi])) for lo, hi in zip(self.bounds[:-1], self.bounds[1:])]
        return stage2(np.array(ranks))


# ---- the solvers -------------------------------------------------------------------------------------------------------
Result = collections.namedtuple("Result", "x iterations state")


def solve2sym(A, RHS):
    """linalg.h:77-88 / solve2sym_dev"""
    f = np.float64
    dinv = f(1.0) / (f(A[0]) * f(A[1]) - f(A[2]) * f(A[2]))
    i0, i1, i2 = dinv * A[1], dinv * A[0], -dinv * A[2]
    return [i0 * RHS[0] + i2 * RHS[1], i2 * RHS[0] + i1 * RHS[1], i0 * RHS[2] + i2 * RHS[3], i2 * RHS[2] + i1 * RHS[3]]


def cg(F, amul, atmul, b, lam, tol, tree="device", bounds=None):
    """fs_cg (bounds=None) or fs_dist_cg scheme "gather" (bounds = row cuts of A'): x, the iteration count, and the final scalars
    {name: value} of st[] that the solve defined (beta only once an iteration did not converge; a solve of F = 0 defines none of
    alpha).  amul(p) = A p, atmul(y) = A' y."""
    red = Reducer(tree, bounds)
    lam, tol = np.float64(lam), np.float64(tol)
    b = np.asarray(b, np.float64).reshape(F)
    with np.errstate(all="ignore"):
        x, r, p = np.zeros(F), b.copy(), b.copy()
        rsq = red(b * b)                                           # kStepCgStart
        stop = tol * np.sqrt(rsq)
        state = {"done": 0.0, "iter": 0.0, "rsq": rsq, "stop": stop}
        for _ in range(F):
            q = atmul(amul(p))
            q = q + lam * p                                        # cg_shift_dot_dev_kernel
            state["alpha"] = alpha = state["rsq"] / red(q * p)     # kStepCgAlpha
            x = x + alpha * p                                      # cg_update_dev_kernel
            r = r - alpha * q
            rr = red(r * r)
            if np.sqrt(rr) <= stop:                                # kStepCgBeta
                state["done"] = 1.0
                break
            state["beta"] = beta = rr / state["rsq"]
            state["rsq"] = rr
            state["iter"] += 1.0
            p = r + beta * p                                       # cg_direction_dev_kernel
    return Result(x, int(state["iter"]), state)


def cg2(F, amul2, atmul2, B, lam, tol, tree="device"):
    """fs_cg2 / fs_dist_cg2 (row-major F x 2): X, the iteration count and the final st[] scalars (all of them: cg2_dev_init
    writes the whole state).  amul2(P) = A P, atmul2(Y) = A' Y for row-major two-column panels."""
    red = Reducer(tree)
    lam, tol = np.float64(lam), np.float64(tol)
    B = np.asarray(B, np.float64).reshape(F, 2)

    def red3(X, Y):                                                # cg2_dot_kernel and its kin: {a'a, b'b, a'b}
        return [red(X[:, 0] * Y[:, 0]), red(X[:, 1] * Y[:, 1]), red(X[:, 0] * Y[:, 1])]

    with np.errstate(all="ignore"):
        h = red3(B, B)
        norms = [np.sqrt(h[0]), np.sqrt(h[1])]                     # host sqrt, host 1.0 / norm
        inorms = [np.float64(1.0) / norms[0], np.float64(1.0) / norms[1]]
        R = np.stack([B[:, 0] * inorms[0], B[:, 1] * inorms[1]], 1)
        P, X = R.copy(), np.zeros((F, 2))
        RtR = red3(R, R)
        Alpha, Psi = [np.float64(0.0)] * 4, [np.float64(0.0)] * 4
        done, it = 0.0, 0
        for _ in range(F):
            Q = atmul2(amul2(P))
            pa, pb = P[:, 0], P[:, 1]
            Q = np.stack([Q[:, 0] + lam * pa, Q[:, 1] + lam * pb], 1)
            qa, qb = Q[:, 0], Q[:, 1]
            Alpha = solve2sym(red3(P, Q), [RtR[0], RtR[2], RtR[2], RtR[1]])    # kStepCg2Alpha
            a0, a1, a2, a3 = Alpha
            X = np.stack([X[:, 0] + (a0 * pa + a1 * pb), X[:, 1] + (a2 * pa + a3 * pb)], 1)
            R = np.stack([R[:, 0] - (a0 * qa + a1 * qb), R[:, 1] - (a2 * qa + a3 * qb)], 1)
            n = red3(R, R)
            if n[0] <= tol * tol and n[1] <= tol * tol:                          # kStepCg2Psi
                done = 1.0
                break
            Psi = solve2sym(RtR, [n[0], n[2], n[2], n[1]])
            RtR = n
            it += 1
            s0, s1, s2, s3 = Psi
            P = np.stack([R[:, 0] + s0 * pa + s1 * pb, R[:, 1] + s2 * pa + s3 * pb], 1)
        X = np.stack([X[:, 0] * norms[0], X[:, 1] * norms[1]], 1)                # cg2_dev_finish
    state = {"done": done, "iter": float(it), "tolsq": tol * tol}
    state.update({f"RtR[{i}]": v for i, v in enumerate(RtR)})
    state.update({f"Alpha[{i}]": v for i, v in enumerate(Alpha)})
    state.update({f"Psi[{i}]": v for i, v in enumerate(Psi)})
    return Result(X, it, state)


def state_from_device(st, two):
    """st[] as fs_debug_last_cg_state returns it -> {name: value} like the model's"""
    out = {}
    for name, at in (ST2 if two else ST1).items():
        if isinstance(at, tuple):
            out.update({f"{name}[{i}]": np.float64(st[at[0] + i]) for i in range(at[1])})
        else:
            out[name] = np.float64(st[at])
    return out


# ---- products and comparisons --------------------------------------------------------------------------------------
def csr_products(nrow, ncol, a_csr, t_csr, lib=None):
    """(A p, A' y, A P, A' Y) as storage-order sums (the oracle's csr_mul / csr_mul_n) over the CSR of A (nrow x ncol) and of A'"""
    from oracle import pyoracle as O
    (arp, acc, avv), (trp, tcc, tvv) = a_csr, t_csr
    return (lambda p: O.csr_mul(nrow, arp, acc, avv, np.ascontiguousarray(p), lib=lib),
            lambda y: O.csr_mul(ncol, trp, tcc, tvv, np.ascontiguousarray(y), lib=lib),
            lambda P: O.csr_mul_n(nrow, arp, acc, avv, P, 2, lib=lib),
            lambda Y: O.csr_mul_n(ncol, trp, tcc, tvv, Y, 2, lib=lib))


def same_bits(a, b):
    """equal bits, or NaN in both places (a NaN's sign and payload are the hardware's)"""
    a, b = np.ascontiguousarray(a, np.float64).reshape(-1), np.ascontiguousarray(b, np.float64).reshape(-1)
    if a.shape != b.shape:
        return np.zeros(max(a.size, b.size), bool)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def mismatch(got, want, got_iter=None, want_iter=None, got_state=None, want_state=None):
    """None when x, the iteration count and every scalar both sides define agree bit for bit; else what differs first"""
    gx, wx = np.ravel(got), np.ravel(want)
    if gx.shape != wx.shape:
        return f"x shape {gx.shape} != {wx.shape}"
    msgs = []
    if got_iter != want_iter:
        msgs.append(f"iterations {got_iter} != {want_iter}")
    if got_state is not None and want_state is not None:
        for k, w in want_state.items():
            if w is None or k not in got_state:
                continue
            if not same_bits(got_state[k], w)[0]:
                msgs.append(f"first differing scalar {k}: got {float(got_state[k])!r} want {float(w)!r}")
                break
    ok = same_bits(gx, wx)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        msgs.append(f"x: {int((~ok).sum())} of {gx.size} differ; first at {i}: got {gx[i]!r} ({gx[i].hex()}) "
                    f"want {wx[i]!r} ({wx[i].hex()})")
    if not msgs:
        return None
    return f"{'; '.join(msgs)} (iterations: got {got_iter}, model {want_iter})"


# ---- the systems -------------------------------------------------------------------------------------------------------
class System:
    """(A'A + lam I) x = b: A as COO (rows, cols[, vals]) in the order a caller hands it over, b (F) and B (F x 2).
    converges: the solve meets ||r|| <= tol ||b|| (the default-mode bars apply); well: well-conditioned (iteration count within
    one); nan: the outcome is NaN (the reference's behaviour, kept)"""

    def __init__(self, name, nrow, ncol, rows, cols, vals, b, B, lam, tol, converges=True, well=True, nan=False, two=True):
        self.name, self.nrow, self.ncol = name, nrow, ncol
        self.rows, self.cols = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(cols, np.int32)
        self.vals = None if vals is None else np.ascontiguousarray(vals, np.float64)
        self.b = np.ascontiguousarray(b, np.float64)
        self.B = None if B is None else np.ascontiguousarray(B, np.float64).reshape(ncol, 2)
        self.lam, self.tol = float(lam), float(tol)
        self.converges, self.well, self.nan, self.two = converges, well, nan, two and B is not None

    def __repr__(self):
        return self.name

    def a_csr(self):
        from oracle import pyoracle as O
        return O.coo_to_csr(self.nrow, self.rows, self.cols, self.vals)

    def t_csr_coo(self):
        """A' as fs_coo_create(ncol, nrow, cols, rows) holds it: every row in the caller's entry order"""
        from oracle import pyoracle as O
        return O.coo_to_csr(self.ncol, self.cols, self.rows, self.vals)

    def t_csr_sorted(self):
        """A' as fs_dist_matrix_build_transpose holds it: every row of A' in ascending A-row order (of the CSR of A)"""
        from oracle import pyoracle as O
        rp, cc, vv = self.a_csr()
        rows = np.repeat(np.arange(self.nrow, dtype=np.int32), np.diff(rp))
        return O.coo_to_csr(self.ncol, cc, rows, vv)

    def model(self, two=False, tree="device", t_csr=None, bounds=None):
        am, atm, am2, atm2 = csr_products(self.nrow, self.ncol, self.a_csr(), t_csr or self.t_csr_coo())
        if two:
            return cg2(self.ncol, am2, atm2, self.B, self.lam, self.tol, tree)
        return cg(self.ncol, am, atm, self.b, self.lam, self.tol, tree, bounds)


def _rhs(F, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(F), rng.standard_normal((F, 2))


def _binary(name, F, nrow, per_row, lam, tol, seed, **kw):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(nrow), per_row)
    cols = rng.integers(0, F, rows.size)
    perm = rng.permutation(rows.size)                         # a caller's COO need not be row-sorted
    b, B = _rhs(F, seed + 1)
    return System(name, nrow, F, rows[perm], cols[perm], None, b, B, lam, tol, **kw)


def systems(large=True):
    """every system of the bit-for-bit tests, by name"""
    import _synth as S
    out = []
    nrow, ncol, rows, cols, _ = S.fixture_sbm()
    i = np.arange(ncol, dtype=np.float64)
    b1, b2 = np.sin(i * 19 + 0.4) + np.cos(i * i * 3), np.cos(i * 23 + 0.7) + np.sin(i * i * 7)     # _cases.cg_rhs
    out.append(System("fixture_100x50", nrow, ncol, rows, cols, None, b1, np.stack([b1, b2], 1), 5.0, 1e-6))
    for F in (1, 63, 64, 65, 257):
        out.append(_binary(f"binary_F{F}", F, 2 * F + 3, 3, 3.0, 1e-10, seed=F))
    if large:
        out.append(_binary("binary_F262145", 262_145, 300_000, 2, 4.0, 1e-9, seed=7))
        out.append(_binary("binary_F600000", 600_000, 500_000, 2, 4.0, 1e-9, seed=8))
    # ~200 iterations; at tol = 1e-13 the recursive residual stops the solve, the true one stays near 1e-12 (converges=False)
    out.append(_binary("ill_conditioned", 600, 420, 4, 1e-3, 1e-13, seed=9, converges=False, well=False))
    out.append(_binary("cap_tol0", 40, 60, 3, 0.5, 0.0, seed=10, converges=False))
    # F = 3, A'A + I with eigenvalues 1 + {1, 3, 4}: CG ends in three steps; tol between the second and third residual
    b3 = np.array([1.0, 0.3, -0.7])
    out.append(System("three_eigenvalues", 3, 3, [0, 0, 1, 1, 2], [0, 1, 1, 2, 2], None, b3,
                      np.stack([b3, [0.2, -1.1, 0.5]], 1), 1.0, 1e-9))
    F = 64
    zb = _binary("zero_rhs", F, 100, 3, 2.0, 1e-8, seed=11, converges=False, nan=True)
    zb.b = np.zeros(F)
    zb.two = False
    out.append(zb)
    z2 = _binary("cg2_zero_column", F, 100, 3, 2.0, 1e-8, seed=12, converges=False, nan=True)
    z2.B[:, 1] = 0.0
    out.append(z2)
    e2 = _binary("cg2_equal_columns", F, 100, 3, 2.0, 1e-8, seed=13, converges=False, nan=True)
    e2.B[:, 1] = e2.B[:, 0]
    out.append(e2)
    # lambda = 0 and column 5 of A empty: r[5] = b[5] for ever, the cap ends the solve
    s = _binary("lambda0_empty_column", 80, 200, 3, 0.0, 1e-8, seed=14, converges=False, well=False)
    s.cols[s.cols == 5] = 6
    out.append(s)
    rng = np.random.default_rng(15)
    v = _binary("valued", 1000, 1500, 4, 2.0, 1e-10, seed=15)
    v.vals = np.where(rng.uniform(size=v.rows.size) < 0.5, -1.0, 1.0) * rng.uniform(0.25, 2.0, v.rows.size)
    v.two = False                                              # (bsbm_cg2 and the reference's bsbm_cg are pattern-only)
    out.append(v)
    return {s.name: s for s in out}


def exact_system(m=3, lam=1.0, F=300, seed=16, nrow=None):
    """A'A = m I exactly (binary A, columns touching disjoint rows, m ones each) and m + lam = 2^e, dyadic b and B with disjoint
    supports: every product, every dot in any order of additions is exact, alpha = 2^-e, x = b / 2^e, r = 0 -- the solve stops at
    iteration 0 in every mode.  nrow = 0: A with no rows, x = b / lam (lam a power of two)."""
    rng = np.random.default_rng(seed)
    if nrow == 0:
        rows = cols = np.zeros(0, np.int32)
    else:
        rows = rng.permutation(F * m)
        cols = np.repeat(np.arange(F), m)
        perm = rng.permutation(rows.size)
        rows, cols = rows[perm], cols[perm]
    b = rng.integers(-64, 65, F) * 2.0 ** rng.integers(-6, 7, F)
    b[b == 0] = 0.75
    B = np.zeros((F, 2))
    B[0::2, 0], B[1::2, 1] = b[0::2], b[1::2] * 0.5
    return System(f"exact_m{m}_F{F}" + ("_norows" if nrow == 0 else ""), F * m if nrow is None else nrow, F, rows, cols, None,
                  b, B, lam, 1e-6)


class ExactFamily:
    """exact_system and what goes with it, for solves that are exact under ANY order of additions (the long-lived-handle walks run
    them in whatever mode the option flips have left).  A'A = d I with columns on disjoint rows and d + lam = c a power of two:
      binary   d = 3, lam = 1, c = 4;   valued   the same pattern with values +-2, so that v * v is 4: d = 12, lam = 4, c = 16
    b and every column of a panel are dyadic with few bits, so A p, A'(A p), q + lam p = c p and every dot are exact; alpha is a
    power of two (1 / c without a preconditioner, 1 with Jacobi, 2 / c with the caller's diagonal c / 2), x = b / c, r = +0.0.
      diag     the caller's diagonal: c / 2 everywhere (a power of two that is not Jacobi's; a diagonal that varies along j would make
               r inexact after the first step)
      x0       "exact" b / c: done before the first iteration;  "other" 2 b / c: r = -b, one pass
      ladders  every d + lambda_i a power of two: w = 1 + sigma_i alpha = (d + lambda_i) / c is one, so den, zn, ratio, a_i are exact
      B2       fs_cg2: +-2^a on 256 rows and +-2^a' on 64 other rows: the column norms are powers of two, R = B / norm is dyadic
    tests/test_lifecycle_model.py runs every solver's model on all of this with the device's sums and with serial sums and asserts
    equal bits: what fails there is not used."""

    def __init__(self, valued=False, F=2000, seed=23):
        rng = np.random.default_rng([seed, int(valued)])
        s = exact_system(m=3, lam=4.0 if valued else 1.0, F=F, seed=seed)
        if valued:
            s.vals = np.where(rng.uniform(size=s.rows.size) < 0.5, -2.0, 2.0)
            s.name += "_valued"
        self.s, self.valued, self.F = s, valued, F
        self.d = 12.0 if valued else 3.0
        self.c = self.d + s.lam
        self.diag = np.full(F, self.c / 2)
        top = [2.0 ** e - self.d for e in range(int(np.log2(self.c)) + 1, int(np.log2(self.c)) + 9)]
        self.ladders = {"m1": [s.lam], "m3": [top[0], s.lam, s.lam],
                        "m16": [top[1], s.lam, top[0], top[7], s.lam, top[2], top[3], top[0], top[4], s.lam, top[5], top[6], top[2], top[7],
                                top[1], top[4]]}
        B2 = np.zeros((F, 2))
        at = rng.permutation(F)[:320]
        B2[at[:256], 0] = np.where(rng.uniform(size=256) < 0.5, -0.125, 0.125)
        B2[at[256:], 1] = np.where(rng.uniform(size=64) < 0.5, -4.0, 4.0)
        self.B2 = B2
        self._signs = np.where(rng.uniform(size=(F, 32)) < 0.5, -1.0, 1.0)

    def panel(self, k):
        """dyadic B (F, k): column j is b with signs of its own times 2^(j % 5 - 2); from k >= 2 column k // 2 is zero (frozen from
        the start), from k >= 8 the last one too"""
        B = self.s.b[:, None] * self._signs[:, :k] * 2.0 ** (np.arange(k) % 5 - 2)[None, :]
        if k >= 2:
            B[:, k // 2] = 0.0
        if k >= 8:
            B[:, k - 1] = 0.0
        return np.ascontiguousarray(B)

    def x0(self, B, how):
        """how: "exact", "other", or "mixed" (panels: the columns take turns -- exact, other, a cold column's zeros)"""
        B = np.asarray(B, np.float64)
        if how == "exact":
            return B / self.c
        if how == "other":
            return B * (2.0 / self.c)
        X0 = np.zeros(B.shape)
        X0[:, 0::3], X0[:, 1::3] = B[:, 0::3] / self.c, B[:, 1::3] * (2.0 / self.c)
        return X0

    def a_csr(self):
        order = np.argsort(self.s.rows, kind="stable")
        return _csr_of(self.s.nrow, self.s.rows[order], self.s.cols[order], None if self.s.vals is None else self.s.vals[order])

    def t_csr(self):
        """A' with every row in the caller's entry order, as fs_coo_create(ncol, nrow, cols, rows) holds it"""
        order = np.argsort(self.s.cols, kind="stable")
        return _csr_of(self.s.ncol, self.s.cols[order], self.s.rows[order], None if self.s.vals is None else self.s.vals[order])

    def products(self):
        """(A p, A' y, A P, A' Y) by bincount: exact on this data, so the order of its additions is nobody's business"""
        s = self.s
        w = 1.0 if s.vals is None else s.vals
        am = lambda p: np.bincount(s.rows, weights=w * np.asarray(p, np.float64)[s.cols], minlength=s.nrow)
        atm = lambda y: np.bincount(s.cols, weights=w * np.asarray(y, np.float64)[s.rows], minlength=s.ncol)
        two = lambda f, n: (lambda Pm: np.stack([f(np.asarray(Pm).reshape(n, 2)[:, 0]), f(np.asarray(Pm).reshape(n, 2)[:, 1])], 1))
        return am, atm, two(am, s.ncol), two(atm, s.nrow)


def _csr_of(nrow, rows, cols, vals):
    rp = np.zeros(nrow + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=nrow), out=rp[1:])
    return rp, np.ascontiguousarray(cols, np.int32), None if vals is None else np.ascontiguousarray(vals, np.float64)


_FAMILIES = {}


def exact_family(valued=False, F=2000, seed=23):
    key = (bool(valued), F, seed)
    if key not in _FAMILIES:
        _FAMILIES[key] = ExactFamily(*key)
    return _FAMILIES[key]
