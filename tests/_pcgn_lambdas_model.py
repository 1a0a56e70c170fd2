"""A CPU restatement of fs_pcgn_lambdas (libfastsparse_amd/csrc/fs_cg.hip), for bit-for-bit tests (helper; no test in here).

fs_pcgn_lambdas is fs_pcgn with a lambda per column, so the model of column j IS the model of fs_pcg (tests/_pcg_model.py) on
B[:, j] at lams[j], with X0[:, j] where there is a warm start.  The preconditioner follows the column: Jacobi's diagonal is that of
the column's own lambda, a caller's diagonal is the same for every column.  Nothing new has to be trusted."""
import numpy as np

import _cg_model as M
import _pcg_model as P
import _pcgn_model as N

# the rungs of a sweep, as multiples of a system's own lambda
LADDER = (1.0, 3.0, 10.0, 30.0, 100.0, 1e3, 1e4, 1e6)


def rungs(s, k):
    """lambda_j = s.lam x LADDER[j % 8] x (1 + 0.25 (j // 8)) for j < k.  A system whose own lambda is 0 keeps exactly 0.0 on
    rung 0 (the formula's value) and climbs the ladder from 0.5 on the others: one rung exactly 0.0, the rest distinct"""
    base = s.lam if s.lam != 0.0 else 0.5
    out = [base * LADDER[j % 8] * (1.0 + 0.25 * (j // 8)) for j in range(k)]
    if s.lam == 0.0:
        out[0] = 0.0
    return out


def dinv_of_column(t_csr, lam, precond, diag=None):
    """what column j's z = r dinv multiplies by: pcg_dinv_kernel's line on fs_gram_diag(At, lam), or on the caller's diagonal"""
    if precond == P.PRECOND_JACOBI:
        return P.dinv_of(P.gram_diag(t_csr, lam))
    if precond == P.PRECOND_DIAG:
        return P.dinv_of(diag)
    return None


def pcgn_lambdas(F, amul, atmul, B, lams, tol, max_iter, dinvs=None, X0=None, tree="device"):
    """fs_pcgn_lambdas on the row-major F x k panel B: column j is _pcg_model.pcg on B[:, j] at lams[j] with dinvs[j]"""
    B = np.asarray(B, np.float64).reshape(F, -1)
    assert len(lams) == B.shape[1]
    cols = [P.pcg(F, amul, atmul, B[:, j], lams[j], tol, max_iter, None if dinvs is None else dinvs[j],
                  None if X0 is None else np.asarray(X0)[:, j], tree) for j in range(B.shape[1])]
    return N.ResultN(np.stack([c.x for c in cols], 1), [N.info_of(c) for c in cols], cols)


def run(s, B, lams, precond=P.PRECOND_NONE, max_iter=0, X0=None, tol=None, diag=None, cache=None):
    """the model's solve of a System with the panel B and one lambda per column (A' in the caller's entry order).  cache: a dict
    that keeps the solve of a column by its lambda and its bytes, for panels that share columns"""
    t_csr = s.t_csr_coo()
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr)
    tol = s.tol if tol is None else tol
    B = np.asarray(B, np.float64).reshape(s.ncol, -1)
    assert len(lams) == B.shape[1]
    cols = []
    for j in range(B.shape[1]):
        lam = float(lams[j])
        x0 = None if X0 is None else np.ascontiguousarray(np.asarray(X0)[:, j])
        key = (s.name, precond, max_iter, tol, lam, B[:, j].tobytes(), None if x0 is None else x0.tobytes())
        col = None if cache is None else cache.get(key)
        if col is None:
            col = P.pcg(s.ncol, am, atm, B[:, j], lam, tol, max_iter, dinv_of_column(t_csr, lam, precond, diag), x0)
            if cache is not None:
                cache[key] = col
        cols.append(col)
    return N.ResultN(np.stack([c.x for c in cols], 1), [N.info_of(c) for c in cols], cols)
