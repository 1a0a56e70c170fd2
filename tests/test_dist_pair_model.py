"""What tests/test_gpu_dist_pair.py relies on, shown on the CPU: the checks it makes on a pair handle fs_dist_matrix_pair(A, At) can
tell the caller's own A' (every row in the caller's entry order, cut where the caller cut it) from the A' that
fs_dist_matrix_build_transpose[_device] would have built (every row in ascending A-row order, cut by non-zeros).

(a) on six named systems the two transposes differ array for array, and so do the bits of the plain-CG model's x; on `zero_rhs` the
    order differs and x does not, on two systems the order is the same: those run on the GPU and are not counted as evidence;
(b) fs_dist_pcg: for every system and case the GPU file solves, the model on both transposes; every class of solve -- no
    preconditioner, Jacobi, a caller's diagonal, a warm start -- has cases whose bits differ;
(c) scheme 1: the slice model on the caller's cuts differs in bits from the slice model on the cut by non-zeros, so the test sees
    which bounds the device sliced by;
(d) the cut by non-zeros restated here is the one of fs_dist.hip, and capi.dist_matrix_pair exists beside its kin."""
import os
import re

import numpy as np
import pytest

import _cg_model as M
import _dist_pair as DPair
import _dist_pcg_model as DP
import _dist_solvers as DV
import _pcg_model as P
import _solvers as SV

SYSTEMS = DPair.systems()


# ---- (a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DPair.SIX)
def test_the_two_transposes_differ_and_so_does_plain_cg(name):
    s = SYSTEMS[name]
    coo, srt = s.t_csr_coo(), s.t_csr_sorted()
    assert np.array_equal(coo[0], srt[0]) and not DPair.same_arrays(coo, srt), name
    a, b = s.model(False, t_csr=coo), s.model(False, t_csr=srt)
    differ = int((~M.same_bits(a.x, b.x)).sum())
    print(f"{name}: {differ} of {s.ncol} entries of the plain-CG model's x differ between the caller's A' and the sorted A'")
    assert differ >= 1, name


def test_the_systems_that_are_no_evidence():
    for name in DPair.SAME_ORDER:
        assert DPair.same_arrays(SYSTEMS[name].t_csr_coo(), SYSTEMS[name].t_csr_sorted()), name
    for name in DPair.SAME_X:
        s = SYSTEMS[name]
        assert not DPair.same_arrays(s.t_csr_coo(), s.t_csr_sorted())
        assert M.same_bits(s.model(False, t_csr=s.t_csr_coo()).x, s.model(False, t_csr=s.t_csr_sorted()).x).all()
    assert set(DPair.SIX + DPair.SAME_ORDER + DPair.SAME_X) == set(DPair.NAMED)
    assert set(DPair.NAMED + DPair.RECIPES0) == set(DV.ALL) - {"binary_F262145"} == set(SYSTEMS)


# ---- (b) ------------------------------------------------------------------------------------------------------------------
def test_every_class_of_pcg_solve_has_cases_that_differ():
    """the caller's diagonal and x0 are the GPU test's (from the caller's A'), the same for both models: only A' changes.  The recipes
    (300 unknowns, a shuffled COO) are solved in all seven cases; the named systems add to the count where they are quick"""
    assert set(c for cs in DPair.CLASSES.values() for c in cs) == set(range(len(SV.CASES)))
    differ = {}
    for name in DPair.RECIPES0 + ("binary_F65", "cap_tol0"):
        s = SYSTEMS[name]
        coo, srt = s.t_csr_coo(), s.t_csr_sorted()
        for case in range(len(SV.CASES)):
            what, precond, x0, max_iter, diag = DV.case_args(s, case, coo)
            a, b = (DP.run(s, precond, max_iter=max_iter, x0=x0, t_csr=t, diag=diag) for t in (coo, srt))
            differ[(name, case)] = int((~M.same_bits(a.x, b.x)).sum())
    for cls, cases in DPair.CLASSES.items():
        hits = sorted((n, SV.CASES[c][0]) for (n, c), d in differ.items() if c in cases and d >= 1)
        print(f"{cls}: {len(hits)} of {sum(c in cases for _, c in differ)} (system, case) pairs differ in the bits of x")
        assert hits, cls
        assert {n for n, _ in hits} >= set(DPair.RECIPES0), (cls, hits)       # (every recipe is evidence for every class)
    assert all(d >= 1 for d in differ.values()), {k: d for k, d in differ.items() if d == 0}


# ---- (c) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranks", [3, 5])
def test_the_callers_cuts_are_another_computation(ranks):
    hits = []
    for name in ("binary_F65", "cap_tol0", "fixture_100x50", "control_seed0"):
        s = SYSTEMS[name]
        coo = s.t_csr_coo()
        cuts, by_nnz = DPair.cut_bounds(s.ncol, ranks), DPair.nnz_bounds(coo[0], ranks)
        assert cuts != by_nnz and cuts[-1] == by_nnz[-1] == s.ncol
        assert any(a == b for a, b in zip(cuts, cuts[1:])) and (ranks != 3 or cuts[-1] - cuts[-2] == 1), cuts   # an empty slice; a one-row slice
        a, b = s.model(False, t_csr=coo, bounds=cuts), s.model(False, t_csr=coo, bounds=by_nnz)
        d = int((~M.same_bits(a.x, b.x)).sum())
        print(f"{name}, {ranks} ranks: cuts {cuts}, by non-zeros {by_nnz}: {d} of {s.ncol} entries of x differ")
        if d:
            hits.append(name)
        if name == "control_seed0":                          # fs_dist_pcg's slice model as well, Jacobi
            a, b = (DP.run(s, P.PRECOND_JACOBI, t_csr=coo, bounds=bb) for bb in (cuts, by_nnz))
            assert not M.same_bits(a.x, b.x).all(), (name, ranks)
    assert len(hits) >= 1, ranks
    print(f"{ranks} ranks: the slice model tells the cuts apart on {hits}")


def test_cut_rows():
    assert DPair.cut_rows(65, 3) == [0, 64, 1] and DPair.cut_rows(65, 5) == [2, 0, 60, 0, 3] and DPair.cut_rows(7, 1) == [7]
    assert DPair.cut_bounds(65, 5) == [0, 2, 2, 62, 62, 65]
    with pytest.raises(AssertionError):
        DPair.cut_rows(3, 5)                                 # three_eigenvalues has no room for five ranks' cuts


# ---- (d) ------------------------------------------------------------------------------------------------------------------
def test_the_cut_by_non_zeros_is_the_sources():
    with open(os.path.join(M.CSRC, "fs_dist.hip")) as f:
        src = " ".join(f.read().split())
    assert "const int64_t target = nnz * r / n;" in src and "return (int64_t)a < t;" in src      # lower_bound on nnz r / n
    assert "bounds[(size_t)r] = b < bounds[(size_t)r - 1] ? bounds[(size_t)r - 1] : b;" in src
    rp = np.array([0, 0, 5, 5, 6, 9, 9])
    assert DPair.nnz_bounds(rp, 3) == [0, 2, 4, 6] and DPair.nnz_bounds(rp, 1) == [0, 6]
    assert DPair.nnz_bounds(np.array([0, 3]), 5) == [0, 0, 1, 1, 1, 1]
    assert DPair.nnz_bounds(np.zeros(4, np.int64), 3) == [0, 0, 0, 3]


def test_capi_has_the_pair():
    with open(os.path.join(M.ROOT, "libfastsparse_amd", "capi.py")) as f:
        src = f.read()
    assert re.search(r"^def dist_matrix_pair\(A, At\):", src, re.M) and "fs_dist_matrix_pair failed" in src
    assert src.index("def dist_matrix_pair") < src.index("def dist_gram_diag")
