"""A CPU restatement of fs_dist_gram_diag and fs_dist_pcg (libfastsparse_amd/csrc/fs_dist.hip), for bit-for-bit tests (helper; no
test in here).

fs_dist_pcg is fs_pcg (tests/_pcg_model.py, whose lines are repeated here one for one) with another `red`:
  scheme 0 "replicate"  bounds=None: every rank runs fs_pcg's kernels on whole vectors -- the whole-vector reducer, fs_pcg itself;
  scheme 1 "gather"     bounds = the row cuts of A': every rank reduces its slice with stage 1 + stage 2, the rank values are added
                        in rank order by stage 2 (_cg_model.Reducer("device", bounds)); an empty slice is 1024 partials of +0.0.
The sums fs_pcg takes in one pass ({b.b, r.r}; {r.r, r.z}) travel together, but each is a tree of its own, so the model reduces them
one by one.  fs_dist_gram_diag is fs_gram_diag row by row: a row of A' lives on one rank."""
import numpy as np

import _cg_model as M
import _pcg_model as P

# the launchers fs_pcg and fs_dist_pcg share and the scalar steps cg_dev_final learnt; test_dist_pcg_model.py asserts them against
# the sources
LAUNCHERS = ("pcg_dev_dinv", "cg_dev_init", "pcg_dev_init", "pcg_dev_start", "cg_dev_shift_dot", "cg_dev_update", "cg_dev_direction",
             "cg_dev_steps", "pcgn_dev_init", "pcgn_dev_steps")
FINAL_STEPS = ("kStepPcgStart", "kStepPcgRz", "kStepPcgBeta")
SEND_DOUBLES = 2                                          # kCgSendDoubles: sums per rank in one exchange

gram_diag = P.gram_diag
dinv_of = P.dinv_of


def pcg(F, amul, atmul, b, lam, tol, max_iter, dinv=None, x0=None, bounds=None):
    """fs_dist_pcg: _pcg_model.pcg with the slice reducer"""
    red = M.Reducer("device", bounds)
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
        bb, rr = red(b * b), red(r * r)                            # kStepPcgStart over {b.b, r.r} per rank
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
            if np.sqrt(rr) <= stop:                                # kStepPcgBeta over {r.r[, r.z]} per rank
                state["done"] = 1.0
                break
            z = r if dinv is None else r * dinv
            rzn = rr if dinv is None else red(r * z)
            state["beta"] = beta = rzn / state["rsq"]
            state["rsq"] = rzn
            state["iter"] += 1.0
            p = z + beta * p                                       # pcg_direction_kernel / cg_direction_dev_kernel
    return M.Result(x, int(state["iter"]), state)


def run(s, precond=P.PRECOND_NONE, max_iter=0, x0=None, tol=None, t_csr=None, diag=None, bounds=None):
    """the model's solve of a System on the CSR of A and the A' the shards hold (t_csr; default: the caller's entry order)"""
    t_csr = t_csr or s.t_csr_coo()
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr)
    dinv = None
    if precond == P.PRECOND_JACOBI:
        dinv = dinv_of(gram_diag(t_csr, s.lam))
    elif precond == P.PRECOND_DIAG:
        dinv = dinv_of(diag)
    return pcg(s.ncol, am, atm, s.b, s.lam, s.tol if tol is None else tol, max_iter, dinv, x0, bounds)


# bounds with three non-empty slices on which the slice tree and the whole-vector tree give different bits (asserted by
# test_dist_pcg_model.py and again by the GPU test before it relies on it)
DIFFERING_BOUNDS = {"scaled_seed0": [0, 90, 210, 300], "powerlaw_seed0": [0, 20, 110, 300], "control_seed0": [0, 100, 200, 300]}
