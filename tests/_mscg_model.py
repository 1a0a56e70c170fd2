"""A CPU restatement of fs_mscg (libfastsparse_amd/csrc/fs_cg.hip), for bit-for-bit tests (helper; no test in here).

Built on the reductions of tests/_cg_model.py: every line below is one IEEE double operation per element, rounded once, in the
order the kernels perform it -- the arithmetic include/fastsparse_hip.h spells out.  The base system (the smallest lambda) is
fs_cg / fs_pcg without a preconditioner; the per-shift scalars are numpy vectors over the m shifts, one lane per shift as on the
device (one thread per shift)."""
import collections

import numpy as np

import _cg_model as M
import _pcg_model as P

MAX_SHIFTS = 16
TINY = np.ldexp(1.0, -500)                                         # the guard on |zn|
# st[] slots beyond fs_pcg's and the per-shift array (enums above mscg_init_kernel); test_mscg_model.py asserts them against the source
ST_MSCG = dict(P.ST_PCG, aprev=8, bprev=9, nlive=10, nbase=11)
MS = {"sigma": 0, "z": 1, "zp": 2, "zn": 3, "ratio": 4, "a": 5, "b": 6, "rn": 7, "live": 8, "converged": 9, "count": 10, "list": 11,
      "pslot": 12}
MS_STRIDE = 16
MSCG_SOURCE_NAMES = {"kStAprev": 8, "kStBprev": 9, "kStNLive": 10, "kStNBase": 11, "kMsSigma": 0, "kMsZ": 1, "kMsZp": 2, "kMsZn": 3,
                     "kMsRatio": 4, "kMsA": 5, "kMsB": 6, "kMsRn": 7, "kMsLive": 8, "kMsConverged": 9, "kMsCount": 10, "kMsList": 11,
                     "kMsPslot": 12, "kMsStride": MS_STRIDE, "kMscgGroup": 4}

Info = collections.namedtuple("Info", "iterations converged rnorm bnorm")
Result = collections.namedtuple("Result", "X infos state shifts")   # state: st[] by name; shifts: {name: (m,) array} of the per-shift array


def _list(live, sigma, lst):
    """mscg_list: live shifts with sigma = 0 first, then the others, each in the caller's order; only that prefix is written"""
    base = [i for i in range(live.size) if live[i] != 0.0 and sigma[i] == 0.0]
    rest = [i for i in range(live.size) if live[i] != 0.0 and sigma[i] != 0.0]
    lst[:len(base) + len(rest)] = base + rest
    return float(len(base)), float(len(rest))


def mscg(F, amul, atmul, b, lams, tol, max_iter=0, tree="device"):
    """fs_mscg: X (m, F), the m infos, the final scalars {name: value} of st[] that the solve defined and the per-shift array
    {name: (m,) values}.  max_iter <= 0: F.  amul(p) = A p, atmul(y) = A' y."""
    red = M.Reducer(tree)
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


def shifts_from_device(raw, m):
    """the doubles fs_debug_last_mscg_state returns -> {name: (m,) values} like the model's"""
    raw = np.asarray(raw, np.float64)[:m * MS_STRIDE].reshape(m, MS_STRIDE)
    return {name: raw[:, at].copy() for name, at in MS.items()}


def state_from_device(st):
    """st[] as fs_debug_last_cg_state returns it after fs_mscg -> {name: value} like the model's"""
    return {name: np.float64(st[at]) for name, at in ST_MSCG.items()}


def shifts_mismatch(got, want):
    """None when every per-shift scalar agrees bit for bit; else the first that differs"""
    for k, w in want.items():
        ok = M.same_bits(got[k], w)
        if not ok.all():
            i = int(np.flatnonzero(~ok)[0])
            return f"per-shift {k}[{i}]: got {float(got[k][i])!r} want {float(w[i])!r}"
    return None


LADDER = (1.0, 3.0, 10.0, 30.0, 100.0, 1e3, 1e4, 1e6)              # times the system's own lambda


def run(s, lams, max_iter=0, tol=None, tree="device", t_csr=None):
    """the model's solve of a _cg_model.System for the lambdas `lams` (A' in the caller's entry order unless t_csr is given)"""
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr or s.t_csr_coo())
    return mscg(s.ncol, am, atm, s.b, lams, s.tol if tol is None else tol, max_iter, tree)
