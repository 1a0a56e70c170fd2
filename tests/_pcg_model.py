"""A CPU restatement of fs_gram_diag and fs_pcg (libfastsparse_amd/csrc/fs_cg.hip), for bit-for-bit tests (helper; no test in here).

Built on the reductions of tests/_cg_model.py: every line below is one IEEE double operation per element, rounded once, in the
order the kernels perform it.

  fs_gram_diag  one wave per row of A'; lane l adds 0.0 + v v of entries l, l + 64, ... in increasing order (one multiply, one add),
                the 64 lanes fold by the __shfl_xor butterfly, lambda is added last.
  fs_pcg        the arithmetic include/fastsparse_hip.h spells out; `red` is the two-stage sum of fs_cg.  The state it returns uses
                fs_cg's names: "rsq" is r.z (st[kStRsq]); "rr" and "bb" are the new slots kStRr and kStBb."""
import numpy as np

import _cg_model as M

# st[] slots beyond ST1 (enum above final_step_kernel); test_pcg_model.py asserts them against the source
ST_PCG = dict(M.ST1, rr=6, bb=7)
PCG_SOURCE_NAMES = {"kStRr": 6, "kStBb": 7}
PRECOND_NONE, PRECOND_JACOBI, PRECOND_DIAG = 0, 1, 2


def gram_diag(t_csr, lam):
    """fs_gram_diag over the CSR (row_ptr, cols, vals or None) of A': d[j] = lam + sum of v^2 over row j"""
    rp, _, vv = t_csr
    rp = np.asarray(rp, np.int64)
    lens = np.diff(rp)
    rounds = -(-lens // M.WAVE)
    sums = np.zeros(lens.size)                                     # an empty row: 64 lanes of +0.0
    for R in np.unique(rounds[rounds > 0]):                        # rows of R rounds together, lane l of round k = entry 64 k + l
        rows = np.flatnonzero(rounds == R)
        for c in range(0, rows.size, 8192):
            rr = rows[c:c + 8192]
            at = rp[rr][:, None] + np.arange(R * M.WAVE)[None, :]
            live = np.arange(R * M.WAVE)[None, :] < lens[rr][:, None]
            v = np.ones(at.shape) if vv is None else np.asarray(vv, np.float64)[np.where(live, at, 0)]
            sq = np.where(live, v * v, 0.0).reshape(rr.size, R, M.WAVE)
            lane = np.zeros((rr.size, M.WAVE))
            for k in range(R):
                lane = lane + sq[:, k, :]
            sums[rr] = M._wave_tree(lane)
    return sums + np.float64(lam)


def dinv_of(d):
    """pcg_dinv_kernel: 1 / d, 1 where d is 0"""
    d = np.asarray(d, np.float64)
    with np.errstate(all="ignore"):
        return np.where(d == 0.0, 1.0, np.float64(1.0) / d)


def pcg(F, amul, atmul, b, lam, tol, max_iter, dinv=None, x0=None, tree="device"):
    """fs_pcg: x, the iteration count and the final scalars {name: value} of st[] that the solve defined.  dinv=None: no
    preconditioner (z is r); x0=None: cold start; max_iter <= 0: F.  amul(p) = A p, atmul(y) = A' y."""
    red = M.Reducer(tree)
    lam, tol = np.float64(lam), np.float64(tol)
    b = np.asarray(b, np.float64).reshape(F)
    cap = max_iter if max_iter > 0 else F
    with np.errstate(all="ignore"):
        if x0 is None:
            x, r = np.zeros(F), b.copy()
        else:
            x = np.array(x0, np.float64).reshape(F)
            q = atmul(amul(x))
            q = q + lam * x                                        # pcg_init_kernel<true>
            r = b - q
        bb, rr = red(b * b), red(r * r)                            # kStepPcgStart
        stop = tol * np.sqrt(bb)
        state = {"done": 0.0, "iter": 0.0, "stop": stop, "rr": rr, "bb": bb}
        if np.sqrt(rr) <= stop:
            state["done"] = 1.0
            return M.Result(x, 0, state)
        z = r if dinv is None else r * dinv                        # pcg_start_kernel
        p = z.copy()
        state["rsq"] = red(r * z)                                  # kStepPcgRz
        for _ in range(cap):
            q = atmul(amul(p))
            q = q + lam * p                                        # cg_shift_dot_dev_kernel
            state["alpha"] = alpha = state["rsq"] / red(q * p)     # kStepCgAlpha
            x = x + alpha * p                                      # pcg_update_kernel / cg_update_dev_kernel
            r = r - alpha * q
            state["rr"] = rr = red(r * r)
            if np.sqrt(rr) <= stop:                                # kStepPcgBeta
                state["done"] = 1.0
                break
            z = r if dinv is None else r * dinv
            rzn = rr if dinv is None else red(r * z)
            state["beta"] = beta = rzn / state["rsq"]
            state["rsq"] = rzn
            state["iter"] += 1.0
            p = z + beta * p                                       # pcg_direction_kernel / cg_direction_dev_kernel
    return M.Result(x, int(state["iter"]), state)


def state_from_device(st):
    """st[] as fs_debug_last_cg_state returns it after fs_pcg -> {name: value} like the model's"""
    return {name: np.float64(st[at]) for name, at in ST_PCG.items()}


# ---- the systems a diagonal preconditioner is for ------------------------------------------------------------------------
NROW, NCOL, PER_ROW = 2000, 300, 8


def recipe(kind, seed, nrow=NROW, ncol=NCOL, per_row=PER_ROW):
    """(A'A + lam I) x = b, A nrow x ncol with per_row entries per row, as a _cg_model.System (one right-hand side):
      "scaled"    valued, uniform columns, standard normal values, column j scaled by 10^U(-1.5, 1.5); lam 1e-3
      "powerlaw"  binary, column j drawn with probability proportional to 1 / (j + 1); lam 0.5
      "control"   valued like "scaled" without the scaling; lam 1e-3
    tol = 1e-8, b standard normal.  The COO is in a caller's (shuffled) order."""
    rng = np.random.default_rng([seed, {"scaled": 1, "powerlaw": 2, "control": 3}[kind]])
    nnz = nrow * per_row
    rows = np.repeat(np.arange(nrow), per_row)
    if kind == "powerlaw":
        w = 1.0 / (np.arange(ncol) + 1.0)
        cols, vals, lam = rng.choice(ncol, nnz, p=w / w.sum()), None, 0.5
    else:
        cols, vals, lam = rng.integers(0, ncol, nnz), rng.standard_normal(nnz), 1e-3
        if kind == "scaled":
            vals = vals * (10.0 ** rng.uniform(-1.5, 1.5, ncol))[cols]
    perm = rng.permutation(nnz)
    b = rng.standard_normal(ncol)
    return M.System(f"{kind}_seed{seed}", nrow, ncol, rows[perm], cols[perm], None if vals is None else vals[perm], b, None, lam, 1e-8)


def dense(s):
    """A of a System as a dense array (duplicates add)"""
    A = np.zeros((s.nrow, s.ncol))
    np.add.at(A, (s.rows, s.cols), 1.0 if s.vals is None else s.vals)
    return A


def run(s, precond=PRECOND_NONE, max_iter=0, x0=None, tol=None, tree="device", t_csr=None, diag=None):
    """the model's solve of a System: A' in the caller's entry order (fs_coo_create(ncol, nrow, cols, rows)) unless t_csr is given"""
    t_csr = t_csr or s.t_csr_coo()
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr)
    dinv = None
    if precond == PRECOND_JACOBI:
        dinv = dinv_of(gram_diag(t_csr, s.lam))
    elif precond == PRECOND_DIAG:
        dinv = dinv_of(diag)
    return pcg(s.ncol, am, atm, s.b, s.lam, s.tol if tol is None else tol, max_iter, dinv, x0, tree)
