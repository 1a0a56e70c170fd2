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


def _k_column_refs(be, data, k):
    """A X(k) through the backend's k-column product, A' U(k) column by column through its A' product"""
    Y = be.csr_mul_n(data.nrow, data.ncol, data.rows, data.cols, data.vals, data.X(k), k,
                     "csr_A_mul_Bn" if data.vals is not None else "bcsr_A_mul_Bn")
    U = data.U(k)
    Z = np.stack([be.coo_tmul(data.nrow, data.ncol, data.rows, data.cols, data.vals, U[:, j].copy()) for j in range(k)], 1)
    return Y, Z


K_REF = 6            # U(6): every scale 2^(j % 4) and several sign patterns


@pytest.mark.parametrize("data", SETS + [SETS[0].pattern()], ids=lambda d: d.name)
def test_k_column_references_are_the_oracle_bit_for_bit(data):
    """Y(k) = A X(k) against the oracle's csr_mul_n, Z(k) = A' U(k) column by column against its coo_tmul (the serial loop of
    At_mul_B / sdm_At_mul_B)"""
    from oracle import pyoracle as O
    Y, Z = _k_column_refs(_cases.OracleBackend(), data, K_REF)
    rp, cc, vv = O.coo_to_csr(data.nrow, data.rows, data.cols, data.vals)
    assert np.array_equal(rp, data.rp) and np.array_equal(cc, data.cols)
    assert E.bits_equal(data.Y(K_REF), Y), (data.name, E.first_mismatch(data.Y(K_REF), Y))
    assert E.bits_equal(data.Z(K_REF), Z), (data.name, E.first_mismatch(data.Z(K_REF), Z))
    assert E.bits_equal(data.Y(K_REF)[:, :3], data.Y(3)) and E.bits_equal(data.Z(K_REF)[:, 0], data.z())


@pytest.mark.ref
@pytest.mark.skipif(not _refbind.available(), reason="oracle/_ref not built (no reference sources here)")
@pytest.mark.parametrize("data", SETS + [SETS[0].pattern()], ids=lambda d: d.name)
def test_k_column_references_are_the_strict_reference_bit_for_bit(data):
    Y, Z = _k_column_refs(_cases.RefBackend(fast=False), data, K_REF)
    assert E.bits_equal(data.Y(K_REF), Y), (data.name, E.first_mismatch(data.Y(K_REF), Y))
    assert E.bits_equal(data.Z(K_REF), Z), (data.name, E.first_mismatch(data.Z(K_REF), Z))


def test_u_panels_keep_the_edges_of_their_sets():
    """U(k) varies signs and scales and nothing else: the subnormal set's A' sums stay subnormal in every column, the zeros set's
    stay +0.0, the odd set is odd on both sides"""
    d3 = E.subnormal()
    U = d3.U(K_REF)
    assert np.array_equal(np.abs(U[:, 1]), np.abs(d3.u) * 2.0) and (np.signbit(U[:, 1]) != np.signbit(d3.u)).sum() > d3.nrow // 4
    Z = d3.Z(K_REF)
    assert all(((Z[:, j] != 0) & (np.abs(Z[:, j]) < 2.0 ** -1022)).sum() > 100 for j in range(K_REF))
    for d in (E.zeros(), E.zeros(valued=False)):
        assert np.all(d.Z(K_REF).view(np.int64) == 0)
    odd = E.wide_range_odd()
    assert odd.nrow % 2 == 1 and odd.ncol % 2 == 1 and odd.nnz > 0
