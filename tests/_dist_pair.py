"""What tests/test_gpu_dist_pair.py and tests/test_dist_pair_model.py share (helper; no test in here): the systems a pair handle
fs_dist_matrix_pair(A, At) is run on, the caller-chosen cuts of A', and the cut by non-zeros that a built transpose would have.

A pair's transposed side is the caller's own At: every row of A' in the caller's entry order (System.t_csr_coo()), cut where the
caller cut it.  A transpose built by fs_dist_matrix_build_transpose[_device] has every row in ascending A-row order
(System.t_csr_sorted()) and is cut by non-zeros.  The tests are worth something on the systems where the two differ."""
import numpy as np

import _cg_model as M
import _pcg_model as P

# the systems of _solvers.DIST_SET whose two transposes differ, and whose plain-CG model differs in bits between them
SIX = ("binary_F65", "ill_conditioned", "cap_tol0", "cg2_equal_columns", "lambda0_empty_column", "valued")
# entry order differs, the model's x does not (b = 0) / A' has the same order either way
SAME_X = ("zero_rhs",)
SAME_ORDER = ("fixture_100x50", "three_eigenvalues")
NAMED = ("fixture_100x50", "binary_F65", "ill_conditioned", "cap_tol0", "three_eigenvalues", "zero_rhs", "cg2_equal_columns",
         "lambda0_empty_column", "valued")                   # _solvers.DIST_SET without binary_F262145
RECIPES0 = ("scaled_seed0", "powerlaw_seed0", "control_seed0")
ROUTES = ("coo", "cuts", "dev")
# the classes of fs_dist_pcg solves that each need a case whose bits tell the two transposes apart: case numbers of _solvers.CASES
CLASSES = {"no preconditioner": (0,), "Jacobi": (1, 5), "caller's diagonal": (2,), "warm start": (3, 4, 6)}
_SYSTEMS = {}


def systems():
    """name -> System: NAMED and the seed-0 recipes"""
    if not _SYSTEMS:
        named = M.systems(large=False)
        _SYSTEMS.update({n: named[n] for n in NAMED})
        _SYSTEMS.update({n: P.recipe(n.split("_")[0], 0) for n in RECIPES0})
    return _SYSTEMS


def cut_rows(F, ranks):
    """rows of A' per rank as a caller may choose them (fs_dist_csr_create_from_shards): on three ranks an empty shard in front and a
    one-row shard at the end, on five ranks empty shards in the middle"""
    rows = {1: [F], 3: [0, F - 1, 1], 5: [2, 0, F - 5, 0, 3]}[ranks]
    assert sum(rows) == F and min(rows) >= 0, (F, ranks, rows)
    return rows


def cut_bounds(F, ranks):
    return [0] + [int(v) for v in np.cumsum(cut_rows(F, ranks))]


def nnz_bounds(row_ptr, ranks):
    """the cut by non-zeros of fs_dist_csr_create / fs_dist_matrix_build_transpose (nnz_cut in fs_dist.hip): bounds[r] is the first
    row whose row_ptr is >= r / ranks of nnz"""
    rp = np.asarray(row_ptr, np.int64)
    nrow, nnz = rp.size - 1, int(rp[-1])
    bounds = [0]
    for r in range(1, ranks):
        bounds.append(max(bounds[-1], min(nrow, int(np.searchsorted(rp, nnz * r // ranks, side="left")))))
    return bounds + [nrow]


def same_arrays(a, b):
    """two CSRs (row_ptr, cols, vals or None), array for array"""
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)) for x, y in zip(a, b))
