"""A CPU restatement of fs_dist_pcgn_lambdas (libfastsparse_amd/csrc/fs_dist.hip), for bit-for-bit tests (helper; no test in here).

fs_dist_pcgn_lambdas is fs_pcgn_lambdas with fs_dist_pcg's `red`, so the model of column j IS the model of fs_dist_pcg
(tests/_dist_pcg_model.py) on B[:, j] at lams[j] with that column's dinv (tests/_pcgn_lambdas_model.dinv_of_column):
  scheme 0 "replicate"  bounds=None: the whole-vector reducer, fs_pcgn_lambdas itself;
  scheme 1 "gather"     bounds = the row cuts of A': every rank reduces its slice of the column, stage 2 adds the rank values.
Nothing new has to be trusted."""
import numpy as np

import _cg_model as M
import _dist_pcg_model as DP
import _pcgn_lambdas_model as NL
import _pcgn_model as N


def run(s, B, lams, precond=NL.P.PRECOND_NONE, max_iter=0, X0=None, tol=None, diag=None, t_csr=None, bounds=None, cache=None):
    """the model's solve of a System with the panel B and one lambda per column on the CSR of A and the A' the shards hold (t_csr;
    default: the caller's entry order).  cache: a dict that keeps the solve of a column by its lambda, its bytes and the bounds"""
    t_csr = t_csr or s.t_csr_coo()
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr)
    tol = s.tol if tol is None else tol
    B = np.asarray(B, np.float64).reshape(s.ncol, -1)
    assert len(lams) == B.shape[1]
    cols = []
    for j in range(B.shape[1]):
        lam = float(lams[j])
        x0 = None if X0 is None else np.ascontiguousarray(np.asarray(X0)[:, j])
        key = (s.name, precond, max_iter, tol, lam, B[:, j].tobytes(), None if x0 is None else x0.tobytes(),
               None if bounds is None else tuple(bounds), t_csr[1].tobytes(), None if t_csr[2] is None else t_csr[2].tobytes(),
               None if diag is None else np.asarray(diag).tobytes())
        col = None if cache is None else cache.get(key)
        if col is None:
            col = DP.pcg(s.ncol, am, atm, B[:, j], lam, tol, max_iter, NL.dinv_of_column(t_csr, lam, precond, diag), x0, bounds)
            if cache is not None:
                cache[key] = col
        cols.append(col)
    return N.ResultN(np.stack([c.x for c in cols], 1), [N.info_of(c) for c in cols], cols)


def columns_that_differ(a, b):
    """how many columns of two solves differ in a bit of X"""
    return int(sum(not M.same_bits(a.X[:, j], b.X[:, j]).all() for j in range(a.X.shape[1])))
