"""tests/_order_model.py on the CPU: hand-built streams whose order of additions can be written down, and the conditions that keep
tests/test_gpu_fixed_order.py from passing emptily -- on every shape it uses the model's bits differ from those of the CSR order
and of the plain stream order in at least one row in ten, shape S has no two entries of a row in one LDS instruction, shape L many."""
import numpy as np
import pytest

import _exact as E
import _order_model as O


def _mat(nrow, ncol, per_row, seed=1):
    """a Data on the rows' column lists `per_row`, values and x that round"""
    rows = np.repeat(np.arange(nrow), [len(c) for c in per_row])
    cols = np.array([c for r in per_row for c in r], np.int64)
    return O.round_data("hand", nrow, ncol, rows, cols, seed)


def _geo(nrow, bcols, kw=1):
    return dict(kw=kw, bcols=bcols, ge=16 // kw, panel_row=np.array([0, nrow], np.int64))


def _seq(d, row, order, x=None, valued=True):
    """0.0 + the row's terms, one rounded add at a time, in the order of `order` (indices into the row's stored entries)"""
    x = d.x if x is None else x
    at = int(d.rp[row])
    s = np.float64(0.0)
    for i in order:
        t = np.float64(x[d.cols[at + i]])
        if valued:
            t = t * np.float64(d.vals[at + i])
        s = s + t
    return s


def _row_positions(d, geo, row):
    return [int(p) for p in O.positions(d, geo)[1][d.rp[row]:d.rp[row + 1]]]


def test_five_entries_at_positions_5_to_9():
    """lane 0 holds 0..7, lane 1 holds 8..15: add i takes entry 8 lane + i of every lane, so 8, 9 (i = 0, 1) come before 5, 6, 7"""
    d = _mat(2, 64, [[9, 3, 60, 17, 2], [40, 1, 33, 8, 21]], seed=2)
    geo = _geo(2, 64)
    assert _row_positions(d, geo, 1) == [5, 6, 7, 8, 9]
    for valued in (True, False):
        y = O.two_pass_ordered(d, d.x, valued, geo)
        assert E.bits_equal(y[1], _seq(d, 1, [3, 4, 0, 1, 2], valued=valued))
        assert E.bits_equal(y[0], _seq(d, 0, [0, 1, 2, 3, 4], valued=valued))
        assert E.bits_equal(O.stream_order(d, d.x, valued, geo)[1], _seq(d, 1, [0, 1, 2, 3, 4], valued=valued))
        assert not E.bits_equal(y[1], _seq(d, 1, [0, 1, 2, 3, 4], valued=valued)), "the data cannot tell the two orders apart"
    assert O.collisions(d, geo) == 0


def test_a_row_across_a_step_of_512():
    """positions 500..515: lane 62 holds 496..503, lane 63 504..511; step 0 adds i = 0..3 of lane 63, then i = 4..7 of lanes 62
    and 63 (two lanes of one instruction on one slot: the lane rule), then step 1 adds 512..515"""
    rng = np.random.default_rng(3)
    per_row = [list(rng.integers(0, 64, 4)) for _ in range(125)] + [list(rng.integers(0, 64, 16))]
    d = _mat(126, 64, per_row)
    geo = _geo(126, 64)
    assert _row_positions(d, geo, 125) == list(range(500, 516))
    up = [504, 505, 506, 507, 500, 508, 501, 509, 502, 510, 503, 511, 512, 513, 514, 515]
    down = [504, 505, 506, 507, 508, 500, 509, 501, 510, 502, 511, 503, 512, 513, 514, 515]
    for lane_order, order in (("ascending", up), ("descending", down)):
        y = O.two_pass_ordered(d, d.x, True, geo, lane_order)
        assert E.bits_equal(y[125], _seq(d, 125, [p - 500 for p in order])), lane_order
        for r in (0, 77, 124):                                     # four consecutive entries of one lane: stream order
            assert E.bits_equal(y[r], _seq(d, r, [0, 1, 2, 3]))
    assert O.collisions(d, geo) == 4


def test_a_row_across_a_band():
    """bands of 64 columns: the panel's stream is band 0's cell (padded to 16 slots), then band 1's; a row stored as
    (band 1, band 0, band 1, band 0) is added band 0 first"""
    d = _mat(2, 128, [[70, 3, 100, 5], [1, 65]])
    geo = _geo(2, 64)
    assert _row_positions(d, geo, 0) == [16, 0, 17, 1] and _row_positions(d, geo, 1) == [2, 18]
    y = O.two_pass_ordered(d, d.x, True, geo)
    assert E.bits_equal(y[0], _seq(d, 0, [1, 3, 0, 2])) and E.bits_equal(y[1], _seq(d, 1, [0, 1]))
    assert E.bits_equal(O.storage_order(d, d.x)[0], _seq(d, 0, [0, 1, 2, 3]))


def test_a_cell_of_17_entries_takes_32_slots():
    """the padding closes the cell: band 0's cell of 17 entries takes slots 0..31, band 1's first entry sits at slot 32, and row 17
    (slots 34..41) straddles lanes 4 and 5: 40 and 41 (i = 0, 1 of lane 5) come first"""
    per_row = [[c] for c in range(16)] + [[20, 90, 91], [92, 93, 94, 95, 96, 97, 98, 99]]
    d = _mat(18, 128, per_row)
    geo = _geo(18, 64)
    panel, p = O.positions(d, geo)
    assert not panel.any() and [int(v) for v in p] == list(range(16)) + [16, 32, 33] + list(range(34, 42))
    y = O.two_pass_ordered(d, d.x, True, geo)
    assert E.bits_equal(y[17], _seq(d, 17, [6, 7, 0, 1, 2, 3, 4, 5]))
    assert E.bits_equal(y[16], _seq(d, 16, [0, 1, 2]))             # (slot 16, then 32 and 33: i = 0 of lanes 2 and 4, i = 1 of lane 4)


@pytest.mark.parametrize("k", [2, 4])
def test_k_columns_by_hand(k):
    """EPL = 8 / k entries per lane, steps of 64 EPL, groups of 16 / k: k = 2, positions 2..6 are added 4, 5, 2, 6, 3 (q = 0, 1 of
    lane 1, then q = 2 of lanes 0 and 1, then q = 3); k = 4, positions 1..4 as 2, 4 (q = 0 of lanes 1, 2), 1, 3 (q = 1)"""
    first, own, order = {2: ([5, 6], [9, 1, 30, 2, 8], [2, 3, 0, 4, 1]), 4: ([5], [9, 1, 30, 2], [1, 3, 0, 2])}[k]
    d = _mat(2, 32, [first, own])
    geo = _geo(2, 32, k)
    assert _row_positions(d, geo, 1) == list(range(len(first), len(first) + len(own)))
    X = d.X(k)
    Y = O.two_pass_ordered_k(d, X, k, geo)
    for j in range(k):
        assert E.bits_equal(Y[1, j], _seq(d, 1, order, X[:, j])), (k, j)
    down = O.two_pass_ordered_k(d, X, k, geo, lane_order="descending")
    swapped = {2: [2, 3, 4, 0, 1], 4: [3, 1, 2, 0]}[k]
    for j in range(k):
        assert E.bits_equal(down[1, j], _seq(d, 1, swapped, X[:, j])), (k, j)


def test_round_data_is_what_the_recipe_says():
    for shape in ("S", "L"):
        d = O.data(shape)
        for v in (d.vals, d.x, d.u, d.X(4)):
            m, e = np.frexp(np.abs(v))
            assert np.all(np.isfinite(v)) and np.all(v != 0) and e.min() >= -7 and e.max() <= 9      # |v| in [2^-8, 2^9)
            assert 0.4 < (v < 0).mean() < 0.6
        lens = np.diff(d.rp)
        assert (lens.min(), lens.max()) == ((3, 8) if shape == "S" else (20, 60))
        starts = d.rp[:-1][lens > 1]
        assert (d.cols[starts] > d.cols[starts + 1]).mean() > 0.3, "columns are not sorted inside a row"
    assert np.bincount(O.data("S").cols).max() <= 8


CASES = [(shape, t, k) for shape in ("S", "L") for t in (0, 1) for k in (1, 2, 4)]


@pytest.mark.parametrize("shape,t,k", CASES, ids=[f"{s}-{'At' if t else 'A'}-k{k}" for s, t, k in CASES])
def test_the_data_can_tell_the_orders_apart(shape, t, k):
    """Among the rows of at least 3 entries, the share whose bits differ between the model and a stand-in order (any column) is at
    least one in ten.  Measured, valued / pattern-only, against (stream order, CSR order); on A' the two stand-ins are one order,
    because a stable sort by column leaves every row of A' in ascending A-row order, which is band order:
        S  A   k=1  (0.140, 0.245) / (0.157, 0.277)    k=2  (0.243, 0.501) / (0.277, 0.545)    k=4  (0.288, 0.726) / (0.340, 0.769)
        S  A'  k=1  (0.155, 0.155) / (0.179, 0.179)    k=2  (0.237, 0.237) / (0.271, 0.271)    k=4  (0.226, 0.226) / (0.266, 0.266)
        L  A   k=1  (0.656, 0.749) / (0.752, 0.795)    k=2  (0.808, 0.936) / (0.908, 0.959)    k=4  (0.891, 0.996) / (0.968, 0.998)
        L  A'  k=1  (0.589, 0.589) / (0.673, 0.673)    k=2  (0.742, 0.742) / (0.864, 0.864)    k=4  (0.770, 0.770) / (0.929, 0.929)
    (S with uniformly drawn columns gave 0.069 to 0.089 against the stream order at k = 1 -- there the ORDERS coincide in most
    rows, which no exponent range mends; hence the home bands of _order_model.shape_s.)"""
    d = O.side(shape, t)
    X = d.x if k == 1 else d.X(k)
    for valued in (True, False):
        model = O.plan_of(shape, t, k)(X, valued)
        for order in ("stream", "storage"):
            share = O.differing_share(model, O.plan_of(shape, t, k, order)(X, valued), d)
            print(f"{shape} {'At' if t else 'A'} k={k} {'valued' if valued else 'pattern'} vs {order}: {share:.3f}")
            assert share >= 0.1, (shape, t, k, valued, order, share)


def test_collisions():
    """pairs of entries of one row in one LDS instruction (same step, same entry-in-lane), single-vector copy:
        S  A 0, A' 0 (rows and columns of at most 8 entries: consecutive slots of a cell, distinct entry-in-lane)
        L  A 732 248, A' 618 691 (rows of 20 to 60 entries)
    and the lane rule then decides bits in L (ascending against descending lanes: 48 % / 38 % of the rows of A / A' differ), in none of S.
    The k-column copies of S do have such pairs (k = 2: 9 926 / 12 033, k = 4: 24 469 / 28 052: four and two entries per lane)."""
    for t in (0, 1):
        s, l = O.side("S", t), O.side("L", t)
        assert O.collisions(s, O.geometry(s)) == 0
        n = O.collisions(l, O.geometry(l))
        print("L", "At" if t else "A", n)
        assert n > 100_000
        up, down = O.plan_of("L", t)(l.x), O.plan_of("L", t, lane_order="descending")(l.x)
        assert O.differing_share(up, down, l) >= 0.1
        assert E.bits_equal(O.plan_of("S", t)(s.x), O.plan_of("S", t, lane_order="descending")(s.x))
        for k in (2, 4):
            assert O.collisions(s, O.geometry(s, k)) > 0


def test_shapes_have_the_geometry_they_are_named_for():
    """S: 3 bands and at least 3 panels, cells that are no multiples of 16 (paddings shift positions), on both sides; L: 2 bands;
    neither takes the large-band form or cuts a row"""
    for shape, t, bands in (("S", 0, 3), ("S", 1, 3), ("L", 0, 2), ("L", 1, 2)):
        d = O.side(shape, t)
        geo = O.geometry(d)
        assert geo["bcols"] == 16384 and -(-d.ncol // geo["bcols"]) == bands, (shape, t)
        P = geo["panel_row"].size - 1
        assert P >= (3 if shape == "S" else 2), (shape, t, P)
        panel = np.searchsorted(geo["panel_row"][:-1], d.rows, side="right") - 1
        cells = np.bincount(panel * bands + d.cols // geo["bcols"], minlength=P * bands)
        assert (cells % 16 != 0).any() and (cells > 512).all(), (shape, t, cells)
        for k in (2, 4):
            gk = O.geometry(d, k)
            assert (gk["bcols"], gk["ge"]) == (16384 // k, 16 // k)
