"""A CPU restatement of fs_pcgn (libfastsparse_amd/csrc/fs_cg.hip), for bit-for-bit tests (helper; no test in here).

fs_pcgn runs k independent fs_pcg recurrences that share only the k-column products, so the model of column j IS the model of fs_pcg
(tests/_pcg_model.py) on B[:, j], with X0[:, j] where there is a warm start.  Nothing else."""
import collections

import numpy as np

import _cg_model as M
import _pcg_model as P

MAX_RHS = 32
# st[] of a solve: fs_pcg's slots (column 0's scalars) and the mask of live columns; cs[]: the per-column scalars.
# test_pcgn_model.py asserts them against the source
ST_PCGN = dict(P.ST_PCG, live_mask=12)
PN = {"bb": 0, "rr": 1, "stop": 2, "rz": 3, "alpha": 4, "beta": 5, "count": 6, "live": 7, "converged": 8}
PN_STRIDE = 16
PCGN_SOURCE_NAMES = dict({"kStLiveMask": 12, "kPnStride": PN_STRIDE, "kPcgnTile": 16, "kPcgnGroup": 8, "kPcgnRowsMaxK": 4},
                         **{"kPn" + k.capitalize(): v for k, v in PN.items()})

Info = collections.namedtuple("Info", "iterations converged rnorm bnorm")
ResultN = collections.namedtuple("ResultN", "X infos columns")        # columns: the _cg_model.Result of every column


def pcgn(F, amul, atmul, B, lam, tol, max_iter, dinv=None, X0=None, tree="device"):
    """fs_pcgn on the row-major F x k panel B: column j is _pcg_model.pcg on B[:, j]"""
    B = np.asarray(B, np.float64).reshape(F, -1)
    cols = [P.pcg(F, amul, atmul, B[:, j], lam, tol, max_iter, dinv, None if X0 is None else np.asarray(X0)[:, j], tree)
            for j in range(B.shape[1])]
    return ResultN(np.stack([c.x for c in cols], 1), [info_of(c) for c in cols], cols)


def info_of(col):
    """fs_pcg_info of a column's solve"""
    with np.errstate(all="ignore"):
        return Info(col.iterations, int(col.state["done"]), np.sqrt(col.state["rr"]), np.sqrt(col.state["bb"]))


def run(s, B, precond=P.PRECOND_NONE, max_iter=0, X0=None, tol=None, diag=None, cache=None):
    """the model's solve of a System with the panel B (A' in the caller's entry order).  cache: a dict that keeps the solve of a
    column by its bytes, for panels that share columns"""
    t_csr = s.t_csr_coo()
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr)
    dinv = None
    if precond == P.PRECOND_JACOBI:
        dinv = P.dinv_of(P.gram_diag(t_csr, s.lam))
    elif precond == P.PRECOND_DIAG:
        dinv = P.dinv_of(diag)
    tol = s.tol if tol is None else tol
    B = np.asarray(B, np.float64).reshape(s.ncol, -1)
    cols = []
    for j in range(B.shape[1]):
        x0 = None if X0 is None else np.ascontiguousarray(np.asarray(X0)[:, j])
        key = (s.name, precond, max_iter, tol, B[:, j].tobytes(), None if x0 is None else x0.tobytes())
        col = None if cache is None else cache.get(key)
        if col is None:
            col = P.pcg(s.ncol, am, atm, B[:, j], s.lam, tol, max_iter, dinv, x0)
            if cache is not None:
                cache[key] = col
        cols.append(col)
    return ResultN(np.stack([c.x for c in cols], 1), [info_of(c) for c in cols], cols)


def state_from_device(cs, k):
    """cs[] as fs_debug_last_pcgn_state returns it -> one {name: value} per column"""
    cs = np.asarray(cs, np.float64).reshape(-1)
    return [{name: np.float64(cs[j * PN_STRIDE + at]) for name, at in PN.items()} for j in range(k)]


# ---- the eight-column recipe: columns that converge at different iterations ---------------------------------------------------
KIND_ID = {"scaled": 1, "powerlaw": 2, "control": 3}


def recipe8(kind):
    """(_pcg_model.recipe(kind, 0), B of 8 columns): standard normal columns; column 1 scaled by 1e-6 and column 2 by 1e6, column 3
    zero, column 4 the top eigenvector of the dense A'A + lam I"""
    s = P.recipe(kind, 0)
    B = np.random.default_rng([77, KIND_ID[kind]]).standard_normal((s.ncol, 8))
    B[:, 1] *= 1e-6
    B[:, 2] *= 1e6
    B[:, 3] = 0.0
    A = P.dense(s)
    K = A.T @ A + s.lam * np.eye(s.ncol)
    B[:, 4] = np.linalg.eigh(K)[1][:, -1]
    return s, np.ascontiguousarray(B), K
