"""The exact reference of tests/_exact.py against the oracle (every product family, bit for bit) and, under -m ref, against the
real reference built without -ffast-math (oracle/_ref/libfsref.so): what "exact" means in tests/test_gpu_exact.py is what
the reference computes, +0.0 and subnormals included, and not only what arithmetic says."""
import numpy as np
import pytest

import _cases
import _exact as E
import _refbind

SETS = E.all_sets()


def _check_all(got, want, who):
    assert got.keys() == want.keys(), (who, sorted(set(got) ^ set(want)))
    bad = [f"{k}: {E.first_mismatch(got[k], want[k])}" for k in sorted(got) if not E.bits_equal(got[k], want[k])]
    assert not bad, (who, bad)


@pytest.mark.parametrize("data", SETS, ids=lambda d: d.name)
def test_exact_reference_is_the_oracle_bit_for_bit(data):
    case = data.case()
    _check_all(_cases.run_case(_cases.OracleBackend(), case), _cases.run_case(E.ExactBackend(), case), data.name)


@pytest.mark.ref
@pytest.mark.skipif(not _refbind.available(), reason="oracle/_ref not built (no reference sources here)")
@pytest.mark.parametrize("data", SETS, ids=lambda d: d.name)
def test_exact_reference_is_the_strict_reference_bit_for_bit(data):
    case = data.case()
    _check_all(_cases.run_case(_cases.RefBackend(fast=False), case), _cases.run_case(E.ExactBackend(), case), data.name)


def test_data_sets_reach_the_edges_they_are_for():
    """the sets hold what their names promise: terms below the 1e-12 bar, rows of 50 000, subnormal sums and sums that cross
    2^-1022, -0.0 products whose sums are +0.0"""
    d1 = E.wide_range()
    p = np.abs(d1.vals * d1.x[d1.cols])
    lo, hi = np.full(d1.nrow, np.inf), np.zeros(d1.nrow)
    np.minimum.at(lo, d1.rows, p)
    np.maximum.at(hi, d1.rows, p)
    two = np.diff(d1.rp) >= 2
    assert np.all(lo[two] / hi[two] == 2.0 ** -46)
    assert max(np.diff(E.long_rows().rp)) == 50_000 and max(np.diff(E.long_rows(profile="heavy", nrow=4000, seed=6).rp)) == 50_000
    d3 = E.subnormal()
    assert np.all(np.abs(d3.vals * d3.x[d3.cols]) < 2.0 ** -1022)
    y = d3.y()
    assert ((y != 0) & (np.abs(y) < 2.0 ** -1022)).sum() > 1000 and (np.abs(y) >= 2.0 ** -1022).sum() > 100
    assert (np.abs(d3.z()) < 2.0 ** -1022).sum() > 100
    d3p = E.subnormal_pattern()
    assert np.all(np.abs(d3p.x) < 2.0 ** -1022) and (np.abs(d3p.y()) >= 2.0 ** -1022).sum() > 10
    for d in (E.zeros(), E.zeros(valued=False)):
        prods = (1.0 if d.vals is None else d.vals) * d.x[d.cols]
        assert np.signbit(prods[prods == 0]).sum() > d.nnz // 3
        for out in (d.y(), d.z(), d.Y(4)):
            assert np.all(out.view(np.int64) == 0)
    assert (np.diff(E.zeros().rp) == 1).sum() > 100 and (np.diff(E.zeros().rp) == 0).sum() > 100


def test_exact_sum_refuses_data_that_breaks_the_rule():
    """a sum that is not exact in some order must fail loudly, never give a flaky expectation"""
    with pytest.raises(AssertionError, match="2\\^53"):
        E.exact_sum(np.zeros(2, int), 1, [1.0, 1.0], [1.0, 2.0 ** -53])            # 1 + 2^-53 rounds
    with pytest.raises(AssertionError, match="above"):
        E.exact_sum(np.zeros(3, int), 1, [1.0, 1.0, 1.0], [2.0 ** 52, 2.0 ** 52, 1.0])
    with pytest.raises(AssertionError, match="significant bits"):
        E.exact_sum(np.zeros(1, int), 1, [1.0 + 2.0 ** -30], [1.0 + 2.0 ** -30])
    with pytest.raises(AssertionError, match="below"):
        E.exact_sum(np.zeros(1, int), 1, [2.0 ** -600], [2.0 ** -500])
    y = E.exact_sum(np.array([0, 0, 1, 2, 2]), 4, [-1.0, 1.0, -1.0, 3.0, -3.0], [0.0, -0.0, 0.0, 5e-324, 5e-324])
    assert E.bits_equal(y, np.zeros(4))
    assert E.bits_equal(E.exact_sum(np.zeros(4, int), 1, [1.0] * 4, [2.0 ** -1074] * 3 + [2.0 ** -1022]),
                        np.array([3 * 2.0 ** -1074 + 2.0 ** -1022]))
