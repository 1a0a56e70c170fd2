"""The ORDER in which the fixed-order two-pass kernels add, as plain numpy (helper; no test in here).

Written from the text of spmv_reduce_ordered_kernel and spmm_reduce_ordered_kernel (libfastsparse_amd/csrc/fs_kernels_twopass.hip)
and of the copy builder (fs_copies.hip); nothing the library computes is used but the planners restated in tests/_plan_model.py.

Stream layout (build_binned_impl).  The rows are cut into panels (plan_two_pass_panels), the columns into bands of `bcols`
columns.  A stable sort by (band, panel) from CSR order leaves every (band, panel) cell in CSR order; pass 2 reads a panel's cells
for ascending band (start2[panel * B + band]).  bin_scatter_kernel puts a cell's entry of rank r at slot r of the cell, and
bin_groups_kernel sizes the cell in whole groups of `ge` = 16 / k entries: THE PADDING SITS AT THE END OF EVERY CELL (the slots
behind its last entry keep the arrays' fill: local row 0, the band's zero slot of x, value 0).  A padding slot adds +0.0 to a sum
that is never -0.0 (it starts at +0.0), so it changes no bits -- but it shifts the position of everything behind it.

Order of the adds (one wave per panel).  Position p counts from the panel's first slot.  A lane holds EPL = 8 / k consecutive
entries of a step of 64 EPL entries, and the wave issues one LDS add per entry-in-lane q (FS_ADD8, add8), each taking entry
EPL lane + q of all 64 lanes:
    step = p // (64 EPL),   lane = (p % (64 EPL)) // EPL,   q = p % EPL;        adds happen in ascending (step, q, lane).
A wave's LDS instructions execute in program order, which gives (step, q); the order of two LANES of one instruction that hit
the same slot is the hardware's.  `lane_order` ("ascending" / "descending") is that one assumption; tests/test_gpu_fixed_order.py
holds the measured rule.  Rows that never have two entries in one instruction (`collisions` == 0) do not depend on it.

Terms: a valued term is fl(x[col] * a), rounded on its own (the build uses -ffp-contract=off), a pattern-only term x[col]; y[r]
starts at +0.0 and takes its terms one rounded add at a time.  k columns: column j sums on its own with fl(X[col, j] * a).

Stand-in orders, to show that the data can tell orders apart: `storage_order` (CSR order: what strict_order computes) and
`stream_order` (ascending p: what the comments used to claim).

Out of the model: copies with cut rows (a row above 256 entries), with dummy entries (one-byte ids over row gaps above 255), the
large-band form, the long-row path."""
import numpy as np

import _exact as E
import _plan_model as M

ORDERS = ("model", "stream", "storage")


# ---- data that rounds ------------------------------------------------------------------------------------------------
def _round_values(rng, n):
    """random sign x random 53-bit mantissa x 2^U{-8..8}: finite, normal, never zero; almost every reordering of a sum of three
    or more of them (or of their products) changes bits"""
    m = rng.integers(1 << 52, 1 << 53, n).astype(np.float64)                 # exact: below 2^53
    return E._signs(rng, n) * np.ldexp(m, rng.integers(-8, 9, n) - 52)


def round_data(name, nrow, ncol, rows, cols, seed):
    """values, x, u and the further columns of X on a pattern given in row-major order (columns NOT sorted inside a row)"""
    rng = np.random.default_rng(seed)
    vals, x, u = _round_values(rng, rows.size), _round_values(rng, ncol), _round_values(rng, nrow)
    xcol = lambda j: _round_values(np.random.default_rng(seed * 1000 + j), ncol)   # noqa: E731
    return E.Data(name, nrow, ncol, rows, cols, vals, x, u, xcol)


def shape_s(seed=51):
    """S: 40 000 x 40 000, 3 to 8 entries per row, at most 8 per column: 3 bands, 4 panels.  A row's (and a column's) entries in
    one cell are consecutive slots, at most 8 of them, so no two share an entry-in-lane q: no row of A or of A' has two entries
    in one instruction, and the model needs no assumption about the hardware here (`collisions` == 0 on both sides).
    Seven entries in ten lie in the band of the row's own block (row // 16 384), the rest anywhere: with uniform columns a row
    has one or two entries per cell, the order of the model then IS the order of the stream in more than nine rows in ten
    (measured: bits differ in 7 to 9 % of the rows, whatever the exponents), and a test on such data could not tell the two apart."""
    rng = np.random.default_rng(seed)
    n, band = 40_000, M.K_BIN_COLS
    rows, cols = E._coo(rng.integers(3, 9, n), n, rng)
    lo = rows // band * band
    width = np.minimum(lo + band, n) - lo
    home = rng.uniform(size=rows.size) < 0.7
    cols[home] = lo[home] + rng.integers(0, width[home])
    while True:                                                             # columns above 8 entries: draw their excess again, in the same band
        order = np.argsort(cols, kind="stable")
        deg = np.bincount(cols, minlength=n)
        first = np.concatenate(([0], np.cumsum(deg)))[:-1]
        over = order[np.arange(rows.size) - first[cols[order]] >= 8]
        if over.size == 0:
            break
        blo = cols[over] // band * band
        cols[over] = blo + rng.integers(0, np.minimum(blo + band, n) - blo)
    return round_data("S", n, n, rows, cols, seed + 1)


def shape_l(seed=53):
    """L: 20 000 x 30 000, 20 to 60 entries per row: 2 bands; lanes of one instruction often hit one slot"""
    rng = np.random.default_rng(seed)
    nrow, ncol = 20_000, 30_000
    rows, cols = E._coo(rng.integers(20, 61, nrow), ncol, rng)
    return round_data("L", nrow, ncol, rows, cols, seed + 1)


SHAPES = {"S": shape_s, "L": shape_l}
_DATA = {}


def data(shape):
    if shape not in _DATA:
        _DATA[shape] = SHAPES[shape]()
    return _DATA[shape]


def transposed(d):
    """A' as a Data of its own, every row in ascending A-row order (fs_matrix_build_transpose: a stable sort by column), x and u
    swapped; made once per Data"""
    if "t" not in d._cache:
        order = np.lexsort((d.rows, d.cols))
        d._cache["t"] = E.Data(d.name + "_t", d.ncol, d.nrow, d.cols[order], d.rows[order], None if d.vals is None else d.vals[order],
                               d.u, d.x, d.ucol)
    return d._cache["t"]


def from_csr(name, nrow, ncol, csr):
    """a Data (matrix only) from (row_ptr, cols, vals or None)"""
    rp, cc, vv = csr
    rows = np.repeat(np.arange(nrow), np.diff(np.asarray(rp, np.int64)))
    return E.Data(name, nrow, ncol, rows, np.asarray(cc), vv, None, None, None)


# ---- geometry and positions ---------------------------------------------------------------------------------------------
def geometry(d, kw=1, ncu=256, big_env=-1, fill=0.8, min_panels=1):
    """what build_binned_impl lays out for d's CSR on a device of `ncu` compute units, for the copy of kw columns"""
    vp, cut = M.virtual_rows(d.rp, 256)
    assert not cut, "a row above 256 entries: cut rows are outside this model"
    g = M.plan_two_pass_geometry(d.nrow, d.ncol, d.nnz, kw, 0, big_env)
    assert not g["big"], "the large-band form is outside this model"
    slots = ncu if ncu > 0 else 256
    panel_row = M.plan_two_pass_panels(vp, d.nrow, d.nnz, g["R"], slots, fill, min_panels, kw)
    return dict(kw=kw, bcols=g["bcols"], ge=g["ge"], panel_row=np.asarray(panel_row, np.int64))


def positions(d, geo):
    """(panel, p) of every entry, in d's CSR order: p counts the slots from the panel's first one, paddings included"""
    rows, cols = d.rows.astype(np.int64), d.cols.astype(np.int64)
    panel_row, bcols, ge = geo["panel_row"], geo["bcols"], geo["ge"]
    B, P = max(1, -(-d.ncol // bcols)), panel_row.size - 1
    panel = np.searchsorted(panel_row[:-1], rows, side="right") - 1
    cell = panel * B + cols // bcols                                        # pass-2 order: panel-major, bands ascending
    count = np.bincount(cell, minlength=P * B)
    padded = -(-count // ge) * ge                                           # the padding closes the cell
    start = np.concatenate(([0], np.cumsum(padded)))[:-1]                   # first slot of every cell, from slot 0 of the stream
    order = np.argsort(cell, kind="stable")                                 # inside a cell: CSR order
    first = np.concatenate(([0], np.cumsum(count)))[:-1]
    rank = np.empty(rows.size, np.int64)
    rank[order] = np.arange(rows.size) - first[cell[order]]
    return panel, start[cell] - start[panel * B] + rank


def order_key(p, geo):
    """(step, q, lane) of position p"""
    epl = 8 // geo["kw"]
    return p // (64 * epl), p % epl, (p % (64 * epl)) // epl


def collisions(d, geo):
    """pairs of entries of one row that share (step, q): two lanes of ONE LDS instruction adding to one slot"""
    panel, p = positions(d, geo)
    step, q, _ = order_key(p, geo)
    key = np.stack([d.rows.astype(np.int64), step, q], 1)                   # (a row lies in one panel)
    _, n = np.unique(key, axis=0, return_counts=True)
    return int((n * (n - 1) // 2).sum())


# ---- sums in a given order ---------------------------------------------------------------------------------------------
class Plan:
    """the entries of d sorted by (row, order of the adds), once; plan(x) then adds rank by rank with whole-array operations: every
    row takes exactly one rounded add per pass, so the sums are the sequential ones"""

    def __init__(self, d, geo=None, order="model", lane_order="ascending"):
        assert order in ORDERS and lane_order in ("ascending", "descending")
        rows = d.rows.astype(np.int64)
        at = np.arange(rows.size)
        if order == "storage":
            perm = np.lexsort((at, rows))
        else:
            _, p = positions(d, geo)                                        # a row's entries share the panel
            if order == "stream":
                perm = np.lexsort((p, rows))
            else:
                step, q, lane = order_key(p, geo)
                perm = np.lexsort((lane if lane_order == "ascending" else -lane, q, step, rows))
        r = rows[perm]
        first = np.concatenate(([0], np.cumsum(np.bincount(r, minlength=d.nrow))))[:-1]
        rank = at - first[r]
        by_rank = np.argsort(rank, kind="stable")
        self.nrow, self.vals = d.nrow, d.vals
        self.src, self.rows = perm[by_rank], r[by_rank]                     # source entry and row of every add, pass by pass
        self.cols = d.cols.astype(np.int64)[self.src]
        self.cut = np.concatenate(([0], np.cumsum(np.bincount(rank, minlength=1))))

    def __call__(self, x, valued=True):
        """y = A x (x of one dimension) or Y = A X (row-major X[ncol, k]) in the plan's order"""
        x = np.asarray(x, np.float64)
        t = x[self.cols]
        if valued and self.vals is not None:
            a = self.vals[self.src]
            t = t * (a if t.ndim == 1 else a[:, None])                      # one rounding; the add below is another
        y = np.zeros((self.nrow,) + x.shape[1:])
        with np.errstate(all="ignore"):
            for a, b in zip(self.cut[:-1], self.cut[1:]):
                y[self.rows[a:b]] = y[self.rows[a:b]] + t[a:b]              # (every row at most once per pass)
        return y


_PLANS = {}


def side(shape, t):
    """A (t = 0) or A' (t = 1) of a shape, as a Data whose x is the vector of that side's product"""
    return transposed(data(shape)) if t else data(shape)


def plan_of(shape, t, k=1, order="model", lane_order="ascending", ncu=256, big_env=-1):
    """the Plan of a shape's side and copy (k = 1, 2, 4), made once per process: the CPU and the GPU tests share it"""
    key = (shape, t, k, order, lane_order if order == "model" else None, ncu if order != "storage" else None, big_env)
    if key not in _PLANS:
        d = side(shape, t)
        _PLANS[key] = Plan(d, None if order == "storage" else geometry(d, k, ncu, big_env), order, lane_order)
    return _PLANS[key]


def two_pass_ordered(d, x, valued, geo, lane_order="ascending"):
    """spmv_reduce_ordered_kernel on d's copy of geometry `geo` (geometry(d, 1, ...))"""
    assert geo["kw"] == 1
    return Plan(d, geo, "model", lane_order)(x, valued)


def two_pass_ordered_k(d, X, k, geo, valued=True, lane_order="ascending"):
    """spmm_reduce_ordered_kernel<V, k, DEPTH> on d's k-column copy of geometry `geo` (geometry(d, k, ...)): row-major Y[nrow, k]"""
    assert geo["kw"] == k and k in (2, 4) and np.shape(X)[1] == k
    return Plan(d, geo, "model", lane_order)(X, valued)


def storage_order(d, x, valued=True):
    """CSR order: 0.0 + t0 + t1 + ...; what strict_order computes"""
    return Plan(d, None, "storage")(x, valued)


def stream_order(d, x, valued, geo):
    """ascending position in the panel's stream: band by band, inside a band in CSR order"""
    return Plan(d, geo, "stream")(x, valued)


def differing_share(a, b, d, min_len=3):
    """among the rows of d with at least min_len entries: the share whose bits differ between a and b (any column)"""
    long = np.diff(np.asarray(d.rp, np.int64)) >= min_len
    a2, b2 = np.asarray(a).reshape(d.nrow, -1), np.asarray(b).reshape(d.nrow, -1)
    differ = (a2.view(np.int64) != b2.view(np.int64)).any(1)
    return float((differ & long).sum()) / float(max(1, long.sum()))
