"""A CPU restatement of fs_dist_mscgn (libfastsparse_amd/csrc/fs_dist.hip), for bit-for-bit tests (helper; no test in here).

fs_dist_mscgn is fs_mscgn with another `red_j`, and fs_mscgn is fs_mscg on every column.  So the model of column j IS the model of
fs_dist_mscg (tests/_dist_mscg_model.py) on B[:, j] with the same `bounds`:
  scheme 0 "replicate"  bounds=None: the whole-vector reducer per column, fs_mscgn itself (tests/_mscgn_model.py);
  scheme 1 "gather"     bounds = the row cuts of A': the slice tree per column.
Nothing else: the pairs' lines are element-wise and do not know about the cuts."""
import numpy as np

import _cg_model as M
import _dist_mscg_model as DS
import _mscgn_model as SN

# the launchers fs_mscgn and fs_dist_mscgn share; test_dist_mscgn_model.py asserts them against the sources
LAUNCHERS = ("mscgn_dev_init", "mscgn_dev_shift_dot", "mscgn_dev_update", "mscgn_dev_direction", "mscgn_dev_steps", "mscgn_dev_rank_step")
SHARED = ("mscg_args_ok", "mscg_shifts", "mscgn_note_state", "mscg_same_outcome")
PROTOTYPE = ("int fs_dist_mscgn(fs_dist_matrix_t M, double *X, int64_t ldx, const double *B, int k, int m, "
             "const double *lambda /* m doubles on the HOST */, double tol, int max_iter, "
             "fs_pcg_info *info /* m * k entries, info[i * k + j], or NULL */);")

ResultN = SN.ResultN
DIFFERING_BOUNDS = DS.DIFFERING_BOUNDS


def _csr_key(csr):
    return tuple(None if a is None else np.ascontiguousarray(a).tobytes() for a in csr)


def run(s, B, lams, max_iter=0, tol=None, t_csr=None, bounds=None, cache=None):
    """the model's solve of a _cg_model.System with the panel B on the CSR of A and the A' the shards hold (t_csr; default: the
    caller's entry order).  cache: a dict that keeps the solve of a column by its bytes, the lambdas, the cap, tol, the bounds and
    the arrays of A'"""
    t_csr = t_csr or s.t_csr_coo()
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr)
    tol = s.tol if tol is None else tol
    B = np.asarray(B, np.float64).reshape(s.ncol, -1)
    tkey = None if cache is None else _csr_key(t_csr)
    cols = []
    for j in range(B.shape[1]):
        key = (s.name, B[:, j].tobytes(), tuple(float(v) for v in lams), max_iter, tol, None if bounds is None else tuple(bounds), tkey)
        col = None if cache is None else cache.get(key)
        if col is None:
            col = DS.mscg(s.ncol, am, atm, B[:, j], lams, tol, max_iter, bounds)
            if cache is not None:
                cache[key] = col
        cols.append(col)
    return SN._gather(cols, len(lams))


def differing_columns(a, b):
    """the columns in which two solves' X differ in at least one bit"""
    return [j for j in range(a.X.shape[2]) if not M.same_bits(a.X[:, :, j], b.X[:, :, j]).all()]
