"""The shapes of tests/_large_bands.py really are what tests/test_gpu_two_pass_large_bands.py needs them to be, on the CPU: the
planner (tests/_plan_model.py, held to fs_plan.h by tests/test_format_plans.py) with the 256 pass-2 slots of an MI355X gives the
large-band form where it is claimed, with bands and panels that cross 16 384; the expected values exist (tests/_exact.py's
exactness rule holds for every product the GPU tests use); and the shapes have teeth: three stand-in faults of a large-band kernel,
computed in numpy, each change at least one row of every product they can touch.  A change of the planner that takes the form, a
tall panel or a wide band away from a shape shows here, not as a silent loss of coverage on the GPU."""
import numpy as np
import pytest

import _exact as E
import _large_bands as LB

BIG, SMALL = LB.BIG, LB.SMALL
SIDES = [(s, t) for s in ("T", "D") for t in (0, 1)]
# what the builder decides by itself for a shape, and the environment the GPU test runs it in (FS_BIN_BIG: -1 unset, 1 forced)
AUTO_BIG, RUN_ENV = {"T": 1, "D": 0}, {"T": -1, "D": 1}


@pytest.fixture(scope="module")
def lay():
    return {(s, t): LB.layout(LB.side(s, True, t), RUN_ENV[s]) for s, t in SIDES}


def test_entries_and_rows_are_what_the_shapes_say():
    t, d = LB.data("T"), LB.data("D")
    assert (t.nrow, t.ncol, t.nnz) == (50_000, 2_000_000, 79_850)
    assert np.all(np.diff(t.rp)[:150] == 200) and np.all(np.diff(t.rp)[150:] == 1)
    assert (d.nrow, d.ncol) == (58_000, 58_000) and 150_000 < d.nnz < 164_000
    lens = np.diff(d.rp)
    assert lens.max() <= 256 and np.all(lens[:256] >= 200) and (lens == 0).sum() > 500         # no cut rows; empty rows exist
    key = d.rows.astype(np.int64) * d.ncol + d.cols
    assert np.all(np.diff(key) > 0)                                                                # row-major, no duplicate entry
    h = d.rows < 256
    assert np.isin(d.cols[h].astype(np.int64) * d.ncol + d.rows[h], key).all()                     # H' is there
    for dd in (t, d):                                                                              # D2 values and vectors
        odd, e, _ = E._split(dd.vals)                                                              # a = +-odd x 2^e
        assert np.abs(odd).max() <= 15 and e.min() >= -4 and e.max() <= 4 and (dd.vals < 0).any() and (dd.vals > 0).any()
        for v in (dd.x, dd.u):
            assert np.all(v == np.round(v)) and np.abs(v).max() <= 1023
    p = LB.data("D", False)
    assert p.vals is None and np.array_equal(p.cols, d.cols) and np.array_equal(p.rp, d.rp)


@pytest.mark.parametrize("shape,t", SIDES)
def test_the_planner_gives_the_large_band_form_where_claimed(lay, shape, t):
    s = LB.side(shape, True, t)
    assert LB.layout(s, -1)["big"] == AUTO_BIG[shape]                    # T: the builder picks it; D: it would not
    L = lay[shape, t]
    assert L["big"] == 1 and L["bcols"] == BIG
    want = {("T", 0): (103, 123, 15_488), ("T", 1): (3, 4, 11_088), ("D", 0): (3, 4, 19_088), ("D", 1): (3, 4, 19_088)}[shape, t]
    assert (L["B"], L["B_small"], L["last_band"]) == want
    assert L["B"] == -(-s.ncol // BIG) != -(-s.ncol // SMALL)
    pr = [int(v) for v in L["panel_rows"]]
    if (shape, t) == ("T", 0):
        assert pr == [100, 9975, 19456, 506, 19456, 507]
        assert 100 < s.nnz / (L["P"] * L["B"]) < 192                    # short runs (about 130 entries)
        assert L["cells"].min() > 0                                       # (uniform columns: no band is empty)
    elif shape == "T":
        assert L["P"] == 256 and max(pr) < SMALL                        # 256 small panels: the min_panels rule
    else:
        assert len(pr) == 6 and pr[2] == pr[4] == BIG
        assert 150 < pr[0] < 250 and 13_000 < pr[1] < 16_000 and 1_500 < pr[3] < 2_600 and 1_500 < pr[5] < 2_600
        assert L["last_band"] % 1024 != 0
        big_cell = int(L["cells"].max())
        assert big_cell > SMALL and big_cell % 16 != 0, big_cell        # whole rounds of both passes plus a guarded rest with padding
        assert big_cell > 2 * 8192


@pytest.mark.parametrize("shape,t", SIDES)
def test_local_ids_cross_16384(lay, shape, t):
    """the ids no ordinary copy ever produces: local columns above 16 383 on every side, local rows above 16 383 on every side
    with a panel of 19 456 rows (T's A' has 256 panels of about 7 800 rows: the min_panels rule)"""
    L = lay[shape, t]
    n_col, n_row = int((L["lcol"] >= SMALL).sum()), int((L["lrow"] >= SMALL).sum())
    assert L["lcol"].max() < BIG and L["lrow"].max() < BIG
    want_col = {("T", 0): (10_000, 15_000), ("T", 1): (5_000, 20_000), ("D", 0): (12_000, 20_000), ("D", 1): (12_000, 20_000)}[shape, t]
    assert want_col[0] < n_col < want_col[1], n_col
    if (shape, t) == ("T", 0):
        assert n_row == 6144                                             # 2 panels x 3 072 rows of one entry
    elif shape == "D":
        assert 8_000 < n_row < 14_000, n_row
    else:
        assert n_row == 0
    if shape == "D" and t == 0:                                          # the columns the non-finite case poisons are referenced
        d = LB.data("D")
        assert (d.cols == LB.NAN_COL).any() and (d.cols == d.ncol - 1).any()


@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
@pytest.mark.parametrize("shape", ["T", "D"])
def test_expected_values_exist(shape, valued):
    """exact_sum asserts the exactness rule while it adds: every product the GPU tests compare against has an exact value"""
    d = LB.data(shape, valued)
    y, z, Y, Z = d.y(), d.z(), d.Y(LB.K), d.Z(LB.K)
    assert y.shape == (d.nrow,) and z.shape == (d.ncol,) and Y.shape == (d.nrow, LB.K) and Z.shape == (d.ncol, LB.K)
    assert E.bits_equal(Y[:, 0], y) and E.bits_equal(Z[:, 0], z)
    assert (y != 0).sum() > 0.8 * (np.diff(d.rp) > 0).sum() and (z != 0).sum() > 1000
    assert not np.signbit(y[np.diff(d.rp) == 0]).any()                  # empty rows: +0.0
    dt = LB.side(shape, valued, 1)
    assert E.bits_equal(dt.y(), z) and E.bits_equal(dt.Y(LB.K), Z)      # the A' side as a matrix of its own: the same sums


def test_the_long_row_set_sits_on_eleven_large_bands():
    d = LB.heavy()
    assert -(-d.ncol // BIG) == 11 and -(-d.ncol // SMALL) == 13 and (np.diff(d.rp) >= 32).sum() > 0


@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
@pytest.mark.parametrize("shape,t", SIDES)
def test_teeth(lay, shape, t, valued):
    """a kernel of this form with a local id masked to 14 bits, with band starts at multiples of 16 384, or that leaves the rows of a
    panel from local row 16 384 on unwritten, gives a product that differs from the exact one in at least one row -- for both
    prefills the GPU tests use.  T's A' has no panel above 16 384 rows, so there the third fault changes nothing (asserted: the
    tall panels of this form are covered by the three other sides)."""
    s = LB.side(shape, valued, t)
    exact = s.y()
    for fill in (np.nan, -0.0):
        for name, y in LB.faults(s, lay[shape, t], fill).items():
            differs = not E.bits_equal(y, exact)
            if name.startswith("rows") and (shape, t) == ("T", 1):
                assert not differs
            else:
                assert differs, (shape, t, valued, name)
                if not name.startswith("rows"):
                    assert (y != exact).sum() >= 10, (name, int((y != exact).sum()))
