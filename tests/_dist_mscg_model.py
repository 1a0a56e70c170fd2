"""A CPU restatement of fs_dist_mscg (libfastsparse_amd/csrc/fs_dist.hip), for bit-for-bit tests (helper; no test in here).

fs_dist_mscg is fs_mscg (tests/_mscg_model.py, whose lines are repeated here one for one) with another `red`:
  scheme 0 "replicate"  bounds=None: every rank runs fs_mscg's kernels on whole vectors -- the whole-vector reducer, fs_mscg itself;
  scheme 1 "gather"     bounds = the row cuts of A': every rank reduces its slice with stage 1 + stage 2, the rank values are added
                        in rank order by stage 2 (_cg_model.Reducer("device", bounds)); an empty slice is 1024 partials of +0.0.
Only the three sums (b.b, q.p, r.r) cross the ranks: S1 and S2 run on every rank over the same gathered values, so the per-shift
scalars, the freezes and the list of live shifts are the same everywhere and the element-wise lines do not know about the cuts."""
import numpy as np

import _cg_model as M
import _mscg_model as S

# the launchers fs_mscg and fs_dist_mscg share and what else they share; test_dist_mscg_model.py asserts them against the sources
LAUNCHERS = ("mscg_dev_init", "mscg_dev_shift_dot", "mscg_dev_update", "mscg_dev_direction", "mscg_dev_steps", "mscg_dev_final")
SHARED = ("mscg_args_ok", "mscg_shifts", "mscg_note_state", "mscg_same_outcome")
PROTOTYPE = ("int fs_dist_mscg(fs_dist_matrix_t M, double *X, int64_t ldx, const double *b, int m, const double *lambda /* host */, "
             "double tol, int max_iter, fs_pcg_info *info /* m entries or NULL */);")

MAX_SHIFTS, TINY, LADDER = S.MAX_SHIFTS, S.TINY, S.LADDER
Info, Result = S.Info, S.Result
_list = S._list


def mscg(F, amul, atmul, b, lams, tol, max_iter=0, bounds=None):
    """fs_dist_mscg: _mscg_model.mscg with the slice reducer"""
    red = M.Reducer("device", bounds)
    f = np.float64
    lams, tol = np.asarray(lams, np.float64).reshape(-1), f(tol)
    m = lams.size
    assert 1 <= m <= MAX_SHIFTS and np.isfinite(lams).all()
    b = np.asarray(b, np.float64).reshape(F)
    cap = max_iter if max_iter > 0 else F
    base = lams.min()                                              # host
    sigma = lams - base
    one, zero = np.ones(m), np.zeros(m)
    with np.errstate(all="ignore"):
        X, r, p = np.zeros((m, F)), b.copy(), b.copy()             # mscg_init_kernel
        pslot = np.full(m, -1.0)
        pslot[sigma != 0.0] = np.arange(int((sigma != 0.0).sum()), dtype=np.float64)
        Pv = {i: b.copy() for i in range(m) if sigma[i] != 0.0}
        bb = red(b * b)                                            # mscg_start_kernel
        stop = tol * np.sqrt(bb)
        done = bool(np.sqrt(bb) <= stop)
        z, zp, zn, ratio, a, bi = one.copy(), one.copy(), one.copy(), one.copy(), zero.copy(), zero.copy()
        rn = np.full(m, np.sqrt(bb))
        live, conv, count = np.full(m, 0.0 if done else 1.0), np.full(m, 1.0 if done else 0.0), zero.copy()
        lst = np.full(m, -1.0)
        state = {"done": 1.0 if done else 0.0, "iter": 0.0, "stop": stop, "rr": bb, "bb": bb, "rsq": bb, "aprev": f(1.0), "bprev": f(0.0),
                 "nbase": 0.0, "nlive": 0.0}
        if not done:
            state["nbase"], state["nlive"] = _list(live, sigma, lst)
        for n in range(cap):
            if state["done"] != 0.0:
                break
            q = atmul(amul(p))
            q = q + base * p                                       # cg_shift_dot_dev_kernel
            state["alpha"] = alpha = state["rsq"] / red(q * p)     # S1
            lv = live != 0.0
            u = alpha * state["bprev"]; u = u * (zp - z)
            w = sigma * alpha; w = 1.0 + w
            v = zp * state["aprev"]; v = v * w
            den = u + v
            t = z * zp; t = t * state["aprev"]; t = t / den
            rat = t / z
            zn, ratio, a = np.where(lv, t, zn), np.where(lv, rat, ratio), np.where(lv, alpha * rat, a)
            r = r - alpha * q                                      # mscg_update_kernel
            rr = red(r * r)
            for i in np.flatnonzero(lv):
                X[i] = X[i] + a[i] * (p if sigma[i] == 0.0 else Pv[i])
            s = np.sqrt(rr)                                        # S2
            state["rr"] = rr
            done = bool(s <= stop)
            beta = rr / state["rsq"]
            if done:
                state["done"] = 1.0
            else:
                state["beta"], state["rsq"], state["aprev"], state["bprev"] = beta, rr, alpha, beta
                state["iter"] += 1.0
            rnn = np.abs(zn) * s
            rn = np.where(lv, rnn, rn)
            freeze = lv & (~(rnn > stop) | (np.abs(zn) < TINY) | done)
            go = lv & ~freeze
            live = np.where(freeze, 0.0, live)
            conv = np.where(freeze, np.where(rnn <= stop, 1.0, 0.0), conv)
            count = np.where(freeze, float(n), np.where(go, float(n + 1), count))
            t = ratio * ratio; t = beta * t
            bi = np.where(go, t, bi)
            zp = np.where(go, z, zp)
            z = np.where(go, zn, z)
            if done:
                break
            state["nbase"], state["nlive"] = _list(live, sigma, lst)
            if state["nbase"] + state["nlive"] == 0.0:
                state["done"] = 1.0
                break
            for i in np.flatnonzero(go):                           # mscg_direction_kernel (the old p is not needed: P of sigma = 0 is p)
                if sigma[i] != 0.0:
                    t1, t2 = z[i] * r, bi[i] * Pv[i]
                    Pv[i] = t1 + t2
            p = r + beta * p
    shifts = {"sigma": sigma, "z": z, "zp": zp, "zn": zn, "ratio": ratio, "a": a, "b": bi, "rn": rn, "live": live, "converged": conv,
              "count": count, "list": lst, "pslot": pslot}
    infos = [Info(int(count[i]), int(conv[i]), f(rn[i]), np.sqrt(bb)) for i in range(m)]
    return Result(X, infos, state, shifts)


def run(s, lams, max_iter=0, tol=None, t_csr=None, bounds=None):
    """the model's solve of a System for the lambdas `lams` on the CSR of A and the A' the shards hold (t_csr; default: the caller's
    entry order)"""
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr or s.t_csr_coo())
    return mscg(s.ncol, am, atm, s.b, lams, s.tol if tol is None else tol, max_iter, bounds)


# bounds with three non-empty slices on which the slice tree and the whole-vector tree give different bits on the m8 ladder (asserted
# by test_dist_mscg_model.py and again by the GPU test before it relies on it)
DIFFERING_BOUNDS = {"control_seed0": [0, 100, 200, 300], "powerlaw_seed0": [0, 20, 110, 300]}
