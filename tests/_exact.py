"""Exactly summable data and an exact reference (no fp64 running sum anywhere).

Exactness rule, per output element: every product a*x is exact in fp64 (mantissa bits of a + mantissa bits of x <= 53,
the product >= 2^-1074, no overflow), and with q the smallest exponent of the last set bit among the element's products,
sum |a*x| <= 2^(q+53).  Then every partial sum, in ANY order, is an integer multiple of 2^q below 2^53 * 2^q: exact.  So
every summation order -- storage order, arrival order, trees, atomics, parts, ranks -- must give the same double, the
exact sum, with +0.0 for a zero sum (the reference starts every sum from `tmp = 0` or a memset: csr.h:431-436).

`exact_sum` checks the rule on the data and fails loudly when it does not hold; a generator that breaks it is a bug.

Data sets (seeded, deterministic), each a `Data` with the matrix in row-major COO / CSR and its vectors (x over columns, u over
rows, the k-column panels X(k) and U(k), and the exact A x, A' u, A X(k), A' U(k)):
  D1 `wide_range`   signed powers of two, <= 64 entries a row, a row's smallest product 2^-46 of its largest;
     `wide_range_odd` the same with an odd number of rows and of columns
  D2 `long_rows`    odd integers 1..15 x 2^[-4, 4] times integers |x| <= 1023, rows of up to 50 000 entries
  D3 `subnormal`    every product of a row a subnormal multiple of 2^-1074; some row sums cross 2^-1022;
     `subnormal_pattern` the pattern-only form with subnormal x
  D4 `zeros`        products -0.0 (-1 * +0.0, +1 * -0.0), rows that cancel exactly, lone -0.0 products, empty rows:
                    every sum is +0.0
"""
import numpy as np

import _cases

# forced copy -> (options at creation, kernel name)
PATHS = {
    "stream": (dict(binning=0, ldsx=0, tiling=0), "stream"),
    "two-pass": (dict(binning=2, bin_flags=64), "two-pass"),
    "two-pass one-byte": (dict(binning=2, bin_flags=128), "two-pass"),
    "long rows": (dict(binning=2, long_rows=2, long_min_len=32), "two-pass"),      # (a copy of >= 4 M entries: test_long_rows_are_exact)
    "lds-staged": (dict(ldsx=2, binning=0, tiling=0), "lds-staged"),
    "tiled cut rows": (dict(tiling=2, binning=0, ldsx=0, tile_rows=64, tile_cols=128, tile_split=5), "tiled"),
}

TWO53 = 2 ** 53


def _split(v):
    """nonzero finite doubles v = s * O * 2^E with O odd: (s * O as int64, E, bit length of O)"""
    m, e = np.frexp(v)
    M = np.abs(m * 2.0 ** 53).astype(np.int64)
    tz = np.frexp((M & -M).astype(np.float64))[1] - 1
    O = M >> tz
    bits = np.frexp(O.astype(np.float64))[1]
    return np.where(v < 0, -O, O), e - 53 + tz, bits


def exact_sum(out, n, a, x):
    """y[o] = sum of a[t] * x[t] over the terms t with out[t] == o, exactly; asserts the exactness rule"""
    out = np.asarray(out, np.int64).reshape(-1)
    a = np.broadcast_to(np.asarray(a, np.float64), out.shape)
    x = np.broadcast_to(np.asarray(x, np.float64), out.shape)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(x)), "exact data holds finite values only"
    y = np.zeros(n)
    nz = (a != 0) & (x != 0)
    out, a, x = out[nz], a[nz], x[nz]
    if out.size == 0:
        return y
    Oa, Ea, Ba = _split(a)
    Ox, Ex, Bx = _split(x)
    assert np.all(Ba + Bx <= 53), "a product with more than 53 significant bits"
    Op, Ep = Oa * Ox, Ea + Ex
    Bp = np.frexp(np.abs(Op).astype(np.float64))[1]
    assert np.all(Ep >= -1074), "a product below 2^-1074"
    assert np.all(Ep + Bp <= 1024), "a product that overflows"
    assert np.array_equal(np.ldexp(Op.astype(np.float64), Ep), a * x), "fp64 products are not the exact ones"
    order = np.argsort(out, kind="stable")
    out, Op, Ep, Bp = out[order], Op[order], Ep[order], Bp[order]
    starts = np.flatnonzero(np.r_[True, out[1:] != out[:-1]])
    q = np.minimum.reduceat(Ep, starts)
    sh = Ep - np.repeat(q, np.diff(np.r_[starts, out.size]))
    assert np.all(sh + Bp <= 53), "a term 2^53 times the smallest last bit of its sum or more"
    T = Op << sh
    # a float guard first so that the int64 sum cannot wrap, then the rule itself on the exact integer sum
    assert np.all(np.add.reduceat(np.abs(T).astype(np.float64), starts) <= 2.0 ** 54), "sum |a x| above 2^(q+53)"
    assert np.all(np.add.reduceat(np.abs(T), starts) <= TWO53), "sum |a x| above 2^(q+53)"
    S = np.add.reduceat(T, starts)
    y[out[starts]] = np.ldexp(S.astype(np.float64), q)          # |S| <= 2^53: converted once, exactly; S == 0 gives +0.0
    return y


def spmv(nrow, rows, cols, vals, x):
    """A x (vals None: pattern-only)"""
    return exact_sum(rows, nrow, 1.0 if vals is None else vals, np.asarray(x)[cols])


def spmv_t(ncol, rows, cols, vals, u):
    """A' u"""
    return exact_sum(cols, ncol, 1.0 if vals is None else vals, np.asarray(u)[rows])


def spmm(nrow, rows, cols, vals, X):
    """A X for row-major X[ncol, k]: the rule holds column by column"""
    X = np.asarray(X).reshape(-1, X.shape[1] if np.ndim(X) == 2 else 1)
    return np.ascontiguousarray(np.stack([spmv(nrow, rows, cols, vals, X[:, j]) for j in range(X.shape[1])], 1))


def ata(nrow, ncol, rows, cols, vals, x, lam=None):
    """A'(A x) (+ lam x): the rule holds for t = A x, then for A' t (with the lam x terms)"""
    t = spmv(nrow, rows, cols, vals, x)
    w = 1.0 if vals is None else vals
    if lam is None:
        return exact_sum(cols, ncol, w, t[rows])
    idx = np.arange(ncol)
    return exact_sum(np.r_[cols, idx], ncol, np.r_[np.broadcast_to(w, cols.shape), np.full(ncol, lam)], np.r_[t[rows], x])


def cbcsr(nrow, rows, cols, x):
    """the column-blocked binary form (cbcsr.h) computes A x of the pattern: blocks change the order, never the sum"""
    return spmv(nrow, rows, cols, None, x)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def first_mismatch(got, want):
    """'index: got (bits) != want (bits)' of the first differing element, for assertion messages"""
    g, w = np.ravel(got), np.ravel(want)
    bad = np.flatnonzero(g.view(np.int64) != w.view(np.int64))
    if bad.size == 0:
        return "equal"
    i = int(bad[0])
    return f"{bad.size} of {g.size} differ; first at {i}: got {g[i]!r} ({g[i].hex()}) want {w[i]!r} ({w[i].hex()})"


# ---- data sets -------------------------------------------------------------------------------------------------
class Data:
    """a matrix (row-major COO + CSR row pointer), x over columns, u over rows, X(k) panels; every product of them obeys the rule"""

    def __init__(self, name, nrow, ncol, rows, cols, vals, x, u, xcol):
        self.name, self.nrow, self.ncol = name, nrow, ncol
        self.rows, self.cols = rows.astype(np.int32), cols.astype(np.int32)
        self.vals = None if vals is None else np.ascontiguousarray(vals, np.float64)
        self.x, self.u, self._xcol = x, u, xcol
        self._cache = {}
        self.rp = np.zeros(nrow + 1, np.int32)
        np.cumsum(np.bincount(self.rows, minlength=nrow), out=self.rp[1:])

    @property
    def nnz(self):
        return int(self.rows.size)

    def X(self, k):
        """row-major ncol x k right-hand sides, column 0 = x"""
        return np.ascontiguousarray(np.stack([self.x] + [self._xcol(j) for j in range(1, k)], 1))

    def ucol(self, j):
        """column j of U: u with seeded per-element sign flips, the whole column scaled by 2^(j % 4).  A flip keeps every |a u| and
        a power of two scales every term of a sum alike (the sets keep their terms far from overflow and, scaled up, from 2^-1074),
        so the exactness rule holds for every column that it holds for with u -- exact_sum checks it all the same."""
        if j == 0:
            return self.u
        return _signs(np.random.default_rng(7000 + j), self.nrow) * self.u * 2.0 ** (j % 4)

    def U(self, k):
        """row-major nrow x k right-hand sides of A' products, column 0 = u"""
        return np.ascontiguousarray(np.stack([self.ucol(j) for j in range(k)], 1))

    def y(self):
        return spmv(self.nrow, self.rows, self.cols, self.vals, self.x)

    def z(self):
        return spmv_t(self.ncol, self.rows, self.cols, self.vals, self.u)

    def Y(self, k):
        """exact A X(k); columns are computed once per data set (X(k) is a prefix of X(k + 1))"""
        cols = self._cache.setdefault("Y", [])
        for j in range(len(cols), k):
            cols.append(spmv(self.nrow, self.rows, self.cols, self.vals, self.x if j == 0 else self._xcol(j)))
        return np.ascontiguousarray(np.stack(cols[:k], 1))

    def Z(self, k):
        """exact A' U(k), column by column"""
        cols = self._cache.setdefault("Z", [])
        for j in range(len(cols), k):
            cols.append(spmv_t(self.ncol, self.rows, self.cols, self.vals, self.ucol(j)))
        return np.ascontiguousarray(np.stack(cols[:k], 1))

    def pattern(self):
        """the same pattern without values (its sums obey the rule on every set built for it: see the set's docstring)"""
        return Data(self.name + "_pattern", self.nrow, self.ncol, self.rows, self.cols, None, self.x, self.u, self._xcol)

    def case(self, kmax=8, block_sizes=(8, 1024), colblocks=(64,)):
        """the data as a tests/_cases.Case: run_case pushes it through every reference-named entry point"""
        d = self
        c = _ExactCase(d.name, d.nrow, d.ncol, d.rows, d.cols, d.vals, {"exact": d.x},
                       block_sizes=block_sizes, colblocks=colblocks, kmax=kmax)
        c.data = d
        c.cg = False
        return c


class _ExactCase(_cases.Case):
    def xt(self, tag):
        return self.data.u

    def X(self, k):
        return self.data.X(k)


class ExactBackend:
    """the exact reference behind the case interface of tests/_cases.py (run_case(ExactBackend(), case))"""

    def coo_mul(self, nrow, ncol, rows, cols, vals, x):
        return spmv(nrow, rows, cols, vals, x)

    def coo_tmul(self, nrow, ncol, rows, cols, vals, x):
        return spmv_t(ncol, rows, cols, vals, x)

    def csr_mul(self, nrow, ncol, rows, cols, vals, x):
        return spmv(nrow, rows, cols, vals, x)

    def csr_mul_n(self, nrow, ncol, rows, cols, vals, X, k, name):
        return spmm(nrow, rows, cols, vals, np.asarray(X).reshape(ncol, k))

    def aa_mul(self, nrow, ncol, rows, cols, x, parallel):
        return ata(nrow, ncol, rows, cols, None, x)

    def blocked_mul(self, nrow, ncol, rows, cols, vals, bs, X, k, name):
        Y = spmm(nrow, rows, cols, vals, np.asarray(X).reshape(ncol, k))
        return Y if k > 1 else Y[:, 0].copy()

    def cbcsr_mul(self, nrow, ncol, rows, cols, cbs, x):
        return cbcsr(nrow, rows, cols, x)


def _coo(lens, ncol, rng):
    rows = np.repeat(np.arange(lens.size), lens)
    return rows, rng.integers(0, ncol, rows.size)


def _signs(rng, n):
    return np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)


def wide_range(seed=1, nrow=2000, ncol=1500, maxlen=64, X0=-3, name="wide_range"):
    """D1: a = +-2^(r_i + w - X0), x = +-2^X0, so a row's products are +-2^(r_i + w), w in [0, 46] with both ends taken in every
    row of two entries or more: the smallest term is 2^-46 of the largest, below the 1e-12 row-scaled bar.  r_i in [-23, 23].
    u_i = +-2^(5 - r_i): a column's products are +-2^(5 - X0 + w), the same 46-bit spread (columns hold < 128 entries), and so
    are the pattern-only column sums of u."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, nrow)
    lens[rng.uniform(size=nrow) < 0.1] = 0
    rows, cols = _coo(lens, ncol, rng)
    r = rng.integers(-23, 24, nrow)
    w = rng.integers(0, 47, rows.size)
    starts = np.r_[0, np.cumsum(lens)[:-1]]
    two = lens >= 2
    w[starts[two]], w[starts[two] + 1] = 0, 46
    vals = _signs(rng, rows.size) * np.ldexp(1.0, r[rows] + w - X0)
    x = _signs(rng, ncol) * 2.0 ** X0
    u = _signs(rng, nrow) * np.ldexp(1.0, 5 - r)
    xcol = lambda j: _signs(np.random.default_rng(seed * 1000 + j), ncol) * 2.0 ** X0        # noqa: E731
    return Data(name, nrow, ncol, rows, cols, vals, x, u, xcol)


def wide_range_odd():
    """D1 with an odd number of rows AND of columns: x (A) and u (A') both have odd length, the LDS-staged kernel's slices of
    either side then go without LDS DMA (it needs an even ncol)"""
    return wide_range(seed=13, nrow=2001, ncol=1499, name="wide_range_odd")


def _odd(rng, n, hi):
    return (2 * rng.integers(0, (hi + 1) // 2, n) + 1).astype(np.float64)


def long_rows(seed=2, nrow=3000, ncol=20000, profile="single", valued=True, maxlen=50_000):
    """D2: a = +-odd(1..15) * 2^[-4, 4], x and u integers |.| <= 1023; `single`: one row of maxlen entries among short ones,
    `heavy`: heavy-tailed lengths up to maxlen"""
    rng = np.random.default_rng(seed)
    if profile == "single":
        lens = rng.integers(0, 20, nrow)
        lens[nrow // 3] = maxlen
    else:
        lens = np.minimum((4 / np.maximum(rng.uniform(size=nrow), 1e-9)).astype(np.int64), maxlen)
        lens[rng.uniform(size=nrow) < 0.05] = 0
        lens[int(np.argmax(lens))] = maxlen
    rows, cols = _coo(lens, ncol, rng)
    vals = _signs(rng, rows.size) * np.ldexp(_odd(rng, rows.size, 15), rng.integers(-4, 5, rows.size)) if valued else None
    x = rng.integers(-1023, 1024, ncol).astype(np.float64)
    u = rng.integers(-1023, 1024, nrow).astype(np.float64)
    xcol = lambda j: np.random.default_rng(seed * 1000 + j).integers(-1023, 1024, ncol).astype(np.float64)   # noqa: E731
    return Data("long_rows_" + profile + ("" if valued else "_pattern"), nrow, ncol, rows, cols, vals, x, u, xcol)


def subnormal(seed=3, nrow=3000, ncol=2500, maxlen=64):
    """D3, valued: x = +-odd(1..3) * 2^[-530, -522]; a = +-odd(1..3) * 2^(p - e_x) puts every product at +-odd(1..9) * 2^p with
    p in [-1074, -1040] (rows that stay subnormal) or p in [-1027, -1026], positive, >= 48 entries (rows whose sum crosses 2^-1022
    back into the normal range).  u_i moves a row's products a * u into [2^-1074, 2^-1028).  X columns: other signs and mantissas,
    the same exponents as x."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, nrow)
    cross = rng.uniform(size=nrow) < 0.15
    lens[cross] = rng.integers(48, maxlen + 1, int(cross.sum()))
    rows, cols = _coo(lens, ncol, rng)
    ex = rng.integers(-530, -521, ncol)
    x = _signs(rng, ncol) * np.ldexp(_odd(rng, ncol, 3), ex)
    p = rng.integers(-1074, -1039, rows.size)
    sgn = _signs(rng, rows.size)
    c = cross[rows]
    p[c] = rng.integers(-1027, -1025, int(c.sum()))
    sgn[c] = 1.0
    sgn[c] *= np.sign(x[cols[c]])                                   # positive products: the sum really crosses 2^-1022
    vals = sgn * np.ldexp(_odd(rng, rows.size, 3), p - ex[cols])
    e_au = p - ex[cols]                                              # exponent of a's last bit
    lo = np.full(nrow, 10 ** 6)
    np.minimum.at(lo, rows, e_au)
    # the smallest a * u of a row at 2^-1074 or (crossing rows) above; u in 2^[-555, -522]: pattern-only sums of u stay exact too
    eu = np.where(lens > 0, np.maximum(-1074 - lo, -555), -540)
    u = _signs(rng, nrow) * np.ldexp(_odd(rng, nrow, 3), eu)

    def xcol(j):
        g = np.random.default_rng(seed * 1000 + j)
        return _signs(g, ncol) * np.ldexp(_odd(g, ncol, 3), ex)
    return Data("subnormal", nrow, ncol, rows, cols, vals, x, u, xcol)


def subnormal_pattern(seed=4, nrow=3000, ncol=2500, maxlen=64):
    """D3, pattern-only: x, u = +-odd(1..3) * 2^[-1060, -1026]; row sums of up to 64 such terms cross 2^-1022 where they are large"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, nrow)
    rows, cols = _coo(lens, ncol, rng)

    def sub(g, n):
        return _signs(g, n) * np.ldexp(_odd(g, n, 3), g.integers(-1060, -1025, n))
    x, u = sub(rng, ncol), sub(rng, nrow)
    x[:ncol // 8] = np.abs(x[:ncol // 8]) * 2.0 ** (-1026 - np.frexp(np.abs(x[:ncol // 8]))[1] + 1)   # a band of large x
    return Data("subnormal_pattern", nrow, ncol, rows, cols, None, x, u, lambda j: sub(np.random.default_rng(seed * 1000 + j), ncol))


def zeros(seed=5, nrow=1200, ncol=900, valued=True):
    """D4: every row sums to zero.  Row kinds: empty; all products -0.0 (value -1 on a column of x = +0.0, value +1 on a
    column of x = -0.0); pairs (a, -a x_c1 / x_c2) that cancel exactly, among -0.0 products; one entry with a -0.0 product.
    u: -0.0 on rows with a positive value, +0.0 on the others.  Pattern-only: x = -0.0 everywhere."""
    rng = np.random.default_rng(seed)
    zc = np.arange(ncol) < ncol // 2                       # columns of x that are zero
    x = np.where(zc, np.where(np.arange(ncol) % 2 == 0, 0.0, -0.0), _signs(rng, ncol) * np.ldexp(1.0, rng.integers(-20, 21, ncol)))
    zcols, nzcols = np.flatnonzero(zc), np.flatnonzero(~zc)
    R, Cc, V = [], [], []
    kind = rng.integers(0, 4, nrow)
    for i in range(nrow):
        if kind[i] == 0:
            continue
        if kind[i] == 3:
            cs = rng.choice(zcols, 1)
        else:
            cs = rng.choice(zcols, int(rng.integers(1, 40)))
        vs = np.where(np.signbit(x[cs]), 1.0, -1.0)
        if kind[i] == 2:
            for _ in range(int(rng.integers(1, 6))):
                c1, c2 = rng.choice(nzcols, 2)
                a1 = float(_signs(rng, 1)[0] * 2.0 ** int(rng.integers(0, 11)) / abs(x[c1]))     # products +-2^[0, 10]
                cs, vs = np.r_[cs, c1, c2], np.r_[vs, a1, -a1 * x[c1] / x[c2]]
        perm = rng.permutation(cs.size)
        R.append(np.full(cs.size, i)), Cc.append(cs[perm]), V.append(vs[perm])
    rows, cols, vals = np.concatenate(R), np.concatenate(Cc), np.concatenate(V)
    pos = np.zeros(nrow, bool)
    np.logical_or.at(pos, rows, vals > 0)
    u = np.where(pos, -0.0, 0.0)
    if not valued:
        x = np.full(ncol, -0.0)
    xcol = lambda j: x * 2.0 ** (j % 8)                    # noqa: E731  (keeps the signs of the zeros)
    return Data("zeros" + ("" if valued else "_pattern"), nrow, ncol, rows, cols, vals if valued else None, x, u, xcol)


def all_sets():
    """the data sets at the small shapes the CPU tests and the entry-point sweep use"""
    return [wide_range(), long_rows(), long_rows(profile="heavy", nrow=4000, seed=6), long_rows(valued=False, seed=7),
            subnormal(), subnormal_pattern(), zeros(), zeros(valued=False), wide_range_odd()]
