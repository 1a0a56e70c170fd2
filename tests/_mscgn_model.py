"""A CPU restatement of fs_mscgn (libfastsparse_amd/csrc/fs_cg.hip), for bit-for-bit tests (helper; no test in here).

fs_mscgn runs fs_mscg on every column of the row-major F x k panel B with scalars of its own; the columns share only the k-column
products.  So the model of column j IS the model of fs_mscg (tests/_mscg_model.py) on B[:, j].  Nothing else."""
import collections

import numpy as np

import _cg_model as M
import _mscg_model as S

MAX_RHS, MAX_SHIFTS = 32, S.MAX_SHIFTS
# sl[], what the flat kernels read per shift (enum above mscgn_step_kernel), and the sizes of the per-column arrays;
# test_mscgn_model.py asserts them against the sources
MSCGN_SOURCE_NAMES = {"kSlNBase": 0, "kSlNLive": 1, "kSlList": 2, "kSlDoubles": 64, "kMscgnListDoubles": 64}
# the sizes that follow the two limits of the header, as the sources spell them
MSCGN_SOURCE_LINES = ("kSlMask = kSlList + kMscgMaxShifts, kSlPslot = kSlMask + kMscgMaxShifts, kSlDoubles = 64",
                      "constexpr int kMscgnStateDoubles = FS_PCGN_MAX_RHS * kMscgStateDoubles;",
                      "constexpr int kMscgnColumnsPerPass = kRedThreads / kMscgMaxShifts;")

ResultN = collections.namedtuple("ResultN", "X infos columns")        # X (m, F, k); infos[i][j]; columns: the _mscg_model.Result of every column


def _gather(cols, m):
    X = np.stack([c.X for c in cols], 2)                               # (m, F, k): panel i is row-major F x k
    return ResultN(X, [[c.infos[i] for c in cols] for i in range(m)], cols)


def mscgn(F, amul, atmul, B, lams, tol, max_iter=0, tree="device"):
    """fs_mscgn on the row-major F x k panel B: column j is _mscg_model.mscg on B[:, j]"""
    B = np.asarray(B, np.float64).reshape(F, -1)
    cols = [S.mscg(F, amul, atmul, B[:, j], lams, tol, max_iter, tree) for j in range(B.shape[1])]
    return _gather(cols, len(lams))


def run(s, B, lams, max_iter=0, tol=None, cache=None):
    """the model's solve of a _cg_model.System with the panel B (A' in the caller's entry order).  cache: a dict that keeps the
    solve of a column by its bytes, for panels that share columns"""
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), s.t_csr_coo())
    tol = s.tol if tol is None else tol
    B = np.asarray(B, np.float64).reshape(s.ncol, -1)
    cols = []
    for j in range(B.shape[1]):
        key = (s.name, tuple(float(v) for v in lams), max_iter, tol, B[:, j].tobytes())
        col = None if cache is None else cache.get(key)
        if col is None:
            col = S.mscg(s.ncol, am, atm, B[:, j], lams, tol, max_iter)
            if cache is not None:
                cache[key] = col
        cols.append(col)
    return _gather(cols, len(lams))
