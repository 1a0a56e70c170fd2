"""The CPU model of fs_mscg (tests/_mscg_model.py), pinned on the CPU:

1  its constants and key lines are the sources';
2  with one lambda it IS the model of fs_pcg without a preconditioner from a cold start (tests/_pcg_model.py), bit for bit: x, the
   count and the state -- so what the shifts add is the only difference; over every system of _cg_model.systems(), with the cap
   of 5 too where ncol <= 1000 (the pure-Python products of the larger ones make a second solve slow; binary_F262145 runs
   uncapped);
3  every column whose lambda is the smallest, duplicates included, IS the model of fs_cg at that lambda, bit for bit; over the
   systems with b != 0 (b = 0 ends before the first iteration: test 2 covers it), tol < 1 (a tol >= 1 system is done at the
   start too) and ncol <= 1000 (run time, as above), plus binary_F262145 for more than one grid stride;
4  on _pcg_model.recipe("control" | "powerlaw") with the ladder lam * {1, 3, 10, 30, 100, 1e3, 1e4, 1e6} against a dense
   numpy.linalg.solve per lambda: every shift converged, true residual <= 2 tol (fs_pcg's bar), the error bound of test_pcg_model.py,
   no shift counts more iterations than the base;
5  freezing: shifts {0, 1e6, 1e9} at tol 1e-14, tol = 0 under a cap, a NaN in r.r;
6  an iteration cap."""
import os

import numpy as np
import pytest

import _cg_model as M
import _mscg_model as S
import _pcg_model as P

SYSTEMS = M.systems()
SEEDS = (0, 1, 2)
KINDS = ("control", "powerlaw")


def test_constants_are_the_sources():
    got = M.source_constants()
    assert {k: got.get(k) for k in S.MSCG_SOURCE_NAMES} == S.MSCG_SOURCE_NAMES
    assert max(S.ST_MSCG.values()) < M.CG_STATE_DOUBLES and got["kStDoubles"] == M.CG_STATE_DOUBLES
    at = list(S.ST_MSCG.values())
    assert len(set(at)) == len(at)                       # the new slots collide with none of fs_cg's and fs_pcg's
    assert sorted(S.MS.values()) == list(range(len(S.MS))) and len(S.MS) <= S.MS_STRIDE
    with open(os.path.join(M.ROOT, "include", "fastsparse_hip.h")) as f:
        hdr = " ".join(f.read().split())
    assert "enum { FS_MSCG_MAX_SHIFTS = 16 };" in hdr and S.MAX_SHIFTS == 16
    assert ("int fs_mscg(fs_matrix_t A, fs_matrix_t At, double *X, int64_t ldx, const double *b, int m, const double *lambda, "
            "double tol, int max_iter, fs_pcg_info *info, fs_stream_t stream);") in hdr
    with open(os.path.join(M.CSRC, "fs_cg.hip")) as f:
        src = " ".join(f.read().split())
    assert "constexpr int kMscgMaxShifts = FS_MSCG_MAX_SHIFTS;" in src
    assert float.fromhex("0x1p-500") == S.TINY


def test_arithmetic_is_the_sources():
    """the lines of fs_cg.hip the model restates"""
    with open(os.path.join(M.CSRC, "fs_cg.hip")) as f:
        src = " ".join(f.read().split())
    for line in ("sg.v[i] = i < m ? lambda[i] - base : 0.0;",
                 "for (int i = 1; i < m; ++i) if (lambda[i] < base) base = lambda[i];",
                 "const int cap = max_iter > 0 ? max_iter : F;",
                 "r[i] = bi; p[i] = bi; for (int j = 0; j < m; ++j) X[j * ldx + i] = 0.0; for (int j = 0; j < nslots; ++j) P[j * ldp + i] = bi; v[0] += bi * bi;",
                 "const double stop = tol * sqrt(bb); const bool done = sqrt(bb) <= stop;",
                 "e[kMsZ] = 1.0; e[kMsZp] = 1.0; e[kMsZn] = 1.0; e[kMsRatio] = 1.0; e[kMsA] = 0.0; e[kMsB] = 0.0;",
                 "e[kMsRn] = sqrt(bb); e[kMsLive] = done ? 0.0 : 1.0; e[kMsConverged] = done ? 1.0 : 0.0; e[kMsCount] = 0.0;",
                 "st[kStAprev] = 1.0; st[kStBprev] = 0.0;",
                 "const double alpha = st[kStRsq] / red[0];",
                 "double u = alpha * bprev; u = u * (zp - z); double w = sigma * alpha; w = 1.0 + w; double v = zp * aprev; v = v * w; "
                 "const double den = u + v; double zn = z * zp; zn = zn * aprev; zn = zn / den; const double ratio = zn / z;",
                 "e[kMsZn] = zn; e[kMsRatio] = ratio; e[kMsA] = alpha * ratio;",
                 "const double ri = r[i] - alpha * q[i]; r[i] = ri; sum += ri * ri;",
                 "for (int u = 0; u < CNT; ++u) xp[u][i] = xv[u] + av[u] * pv[u];",
                 "pp[u] = slot < 0 ? p : P + slot * ldp;",
                 "const double s = sqrt(rr); const bool done = s <= stop; const double beta = rr / rsq;",
                 "else { st[kStBeta] = beta; st[kStRsq] = rr; st[kStIter] = n + 1.0; st[kStAprev] = alpha; st[kStBprev] = beta; }",
                 "const double rn = fabs(zn) * s;",
                 "if (!(rn > stop) || fabs(zn) < 0x1p-500 || done) {",
                 "e[kMsLive] = 0.0; e[kMsConverged] = rn <= stop ? 1.0 : 0.0; e[kMsCount] = n;",
                 "double bi = ratio * ratio; bi = beta * bi; e[kMsB] = bi; e[kMsZp] = e[kMsZ]; e[kMsZ] = zn; e[kMsCount] = n + 1.0;",
                 "if (nb + nl == 0) st[kStDone] = 1.0;",
                 "if (FIRST) p[i] = ri + beta * p[i];",
                 "for (int u = 0; u < CNT; ++u) { const double t1 = zv[u] * ri, t2 = bv[u] * pv[u]; pp[u][i] = t1 + t2; }",
                 "hipLaunchKernelGGL(cg_shift_dot_dev_kernel, g, blk, 0, s, F, base, q, p, part, st);"):
        assert line in src, line


def _products(s):
    return M.csr_products(s.nrow, s.ncol, s.a_csr(), s.t_csr_coo())[:2]


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
PCG_KEYS = ("done", "iter", "stop", "rr", "bb", "rsq", "alpha", "beta")


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_one_lambda_is_the_pcg_model(name):
    s = SYSTEMS[name]
    am, atm = _products(s)
    for cap in (0, 5) if s.ncol <= 1000 else (0,):
        want = P.pcg(s.ncol, am, atm, s.b, s.lam, s.tol, cap)
        got = S.mscg(s.ncol, am, atm, s.b, [s.lam], s.tol, cap)
        bad = M.mismatch(got.X[0], want.x, got.infos[0].iterations, want.iterations, got.state, want.state)
        assert bad is None, (name, cap, bad)
        assert all(k in got.state for k in want.state), (name, sorted(got.state), sorted(want.state))
        assert set(want.state) <= set(PCG_KEYS)
        info = got.infos[0]
        assert info.converged == int(want.state["done"]) and M.same_bits(info.rnorm, np.sqrt(want.state["rr"]))[0]
        assert M.same_bits(info.bnorm, np.sqrt(want.state["bb"]))[0]
        assert got.shifts["z"][0] == 1.0 and got.shifts["sigma"][0] == 0.0 and got.shifts["pslot"][0] == -1.0
        if cap and want.state["done"] == 0.0:
            assert info.iterations == cap
    if name == "zero_rhs":
        assert info.iterations == 0 and info.converged == 1 and M.same_bits(got.X, np.zeros((1, s.ncol))).all()
        assert "alpha" not in got.state


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
BASE_SET = [n for n, s in SYSTEMS.items() if np.any(s.b != 0) and s.tol < 1 and s.ncol <= 1000] + ["binary_F262145"]


@pytest.mark.parametrize("name", BASE_SET)
def test_columns_of_the_smallest_lambda_are_the_cg_model(name):
    s = SYSTEMS[name]
    am, atm = _products(s)
    want = M.cg(s.ncol, am, atm, s.b, s.lam, s.tol)
    lams = [s.lam + 2.0, s.lam, s.lam * 10 + 1.0, s.lam]            # the minimum twice, not in front
    got = S.mscg(s.ncol, am, atm, s.b, lams, s.tol)
    for i in (1, 3):
        keys = {k: v for k, v in want.state.items() if k in ("alpha", "beta", "rsq", "stop", "done", "iter")}
        bad = M.mismatch(got.X[i], want.x, got.infos[i].iterations, want.iterations, got.state, keys)
        assert bad is None, (name, i, bad)
        assert got.infos[i].converged == int(want.state["done"])
        for k, v in (("z", 1.0), ("zp", 1.0), ("zn", 1.0), ("ratio", 1.0), ("sigma", 0.0), ("pslot", -1.0)):
            assert got.shifts[k][i] == v, (name, i, k, got.shifts[k][i])
    assert list(got.shifts["pslot"]) == [0.0, -1.0, 1.0, -1.0]
    for i in (0, 2):
        assert got.infos[i].iterations <= want.iterations and 0.0 < got.shifts["zn"][i] < 1.0, (name, i)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _recipe(kind, seed):
    key = (kind, seed)
    if key not in _RUNS:
        s = P.recipe(kind, seed)
        A = P.dense(s)
        _RUNS[key] = (s, A.T @ A)
    return _RUNS[key]


def _check_against_dense(s, G, lams, got):
    bn = np.linalg.norm(s.b)
    base = int(np.argmin(lams))
    worst = 0.0
    for i, lam in enumerate(lams):
        K = G + lam * np.eye(s.ncol)
        res = lambda x: float(np.linalg.norm(K @ x - s.b) / bn)
        direct = np.linalg.solve(K, s.b)
        assert res(direct) <= 1e-10                                  # the yardstick itself
        info = got.infos[i]
        what = (s.name, i, lam, info, res(got.X[i]))
        assert info.converged == 1, what
        assert res(got.X[i]) <= 2 * s.tol, what
        # ||x - x*|| <= ||K^-1|| ||K x - b|| <= residual ||b|| / lam_min, and lam_min(K) >= lam
        assert np.linalg.norm(got.X[i] - direct) <= (res(got.X[i]) + res(direct)) * bn / lam * 1.01, what
        assert info.iterations <= got.infos[base].iterations, what
        assert info.rnorm <= s.tol * info.bnorm, what
        worst = max(worst, res(got.X[i]) / s.tol)
    return worst


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind", KINDS)
def test_ladder_converges_to_the_dense_solutions(kind, seed):
    s, G = _recipe(kind, seed)
    lams = [s.lam * f for f in S.LADDER]
    got = S.run(s, lams)
    worst = _check_against_dense(s, G, lams, got)
    counts = [i.iterations for i in got.infos]
    print(f"{s.name}: counts {counts}, worst true residual {worst:.2f} tol")
    assert counts == sorted(counts, reverse=True)                    # a larger shift is never later
    assert got.state["done"] == 1.0 and got.state["iter"] == counts[0]
    # shuffled, with a duplicate: the same numbers column by column (the base system does not depend on the order)
    order = [5, 2, 7, 0, 3, 3, 6, 1, 4]
    again = S.run(s, [lams[k] for k in order])
    _check_against_dense(s, G, [lams[k] for k in order], again)
    for col, k in enumerate(order):
        assert M.same_bits(again.X[col], got.X[k]).all() and again.infos[col] == got.infos[k], (s.name, col, k)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_large_shifts_freeze_and_stay_finite(kind):
    s, G = _recipe(kind, 0)
    lams = [0.0, 1e6, 1e9] if kind == "control" else [s.lam, s.lam + 1e6, s.lam + 1e9]
    got = S.run(s, lams, tol=1e-14)
    print(f"{s.name}: {got.infos}")
    assert np.isfinite(got.X).all() and all(np.isfinite(v).all() for v in got.shifts.values())
    assert all(i.converged == 1 for i in got.infos), got.infos
    assert got.infos[2].iterations <= got.infos[1].iterations < got.infos[0].iterations
    bn = np.linalg.norm(s.b)
    for i, lam in enumerate(lams):
        assert np.linalg.norm(G @ got.X[i] + lam * got.X[i] - s.b) <= 1e-12 * bn, (i, lam)


@pytest.mark.parametrize("kind", KINDS)
def test_tol_zero_ends_through_the_guard_or_the_cap(kind):
    s, G = _recipe(kind, 0)
    lams = [0.0, 1e6, 1e9] if kind == "control" else [s.lam, s.lam + 1e6, s.lam + 1e9]
    got = S.run(s, lams, tol=0.0, max_iter=200)
    print(f"{s.name}: {got.infos}, |zn| {np.abs(got.shifts['zn'])}")
    assert np.isfinite(got.X).all() and all(np.isfinite(v).all() for v in got.shifts.values())
    for i, info in enumerate(got.infos):
        capped = info.iterations == 200 and got.shifts["live"][i] == 1.0
        guarded = got.shifts["live"][i] == 0.0 and abs(got.shifts["zn"][i]) < S.TINY and info.iterations < 200
        assert capped != guarded and info.converged == 0, (i, info, got.shifts["zn"][i])
    assert got.shifts["live"][0] == 1.0 and got.shifts["live"][2] == 0.0          # the base runs to the cap, 1e9 does not
    bn = np.linalg.norm(s.b)
    for i, lam in enumerate(lams):
        assert np.linalg.norm(G @ got.X[i] + lam * got.X[i] - s.b) <= 1e-12 * bn, (i, lam)


def test_nan_freezes_every_shift_unconverged():
    s, _ = _recipe("control", 0)
    am, atm = _products(s)
    calls = []

    def poisoned(p):
        calls.append(1)
        y = am(p)
        if len(calls) == 3:
            y = y.copy()
            y[0] = np.nan
        return y

    lams = [s.lam * f for f in (10.0, 1.0, 1e3)]
    got = S.mscg(s.ncol, poisoned, atm, s.b, lams, s.tol)
    assert np.isnan(got.state["rr"]) and len(calls) == 3                           # nothing is enqueued for frozen shifts
    assert all(i.converged == 0 and i.iterations == 2 and np.isnan(i.rnorm) for i in got.infos), got.infos
    assert not got.shifts["live"].any() and got.state["done"] == 1.0 and got.state["nbase"] + got.state["nlive"] == 0.0


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_cap(seed):
    s, G = _recipe("powerlaw", seed)
    lams = [s.lam * f for f in S.LADDER]
    full = S.run(s, lams)
    counts = [i.iterations for i in full.infos]
    cap = counts[5] + 2                                              # shifts 1e3 and beyond are frozen by then, the others are not
    assert counts[4] > cap > counts[5]
    got = S.run(s, lams, max_iter=cap)
    assert got.state["done"] == 0.0 and got.state["iter"] == cap
    for i, info in enumerate(got.infos):
        if counts[i] < cap:
            assert info == full.infos[i] and M.same_bits(got.X[i], full.X[i]).all(), (i, info)
            assert got.shifts["live"][i] == 0.0
        else:
            assert info.iterations == cap and info.converged == 0 and got.shifts["live"][i] == 1.0, (i, info)
            assert info.rnorm > s.tol * info.bnorm
    # the capped solve is the first `cap` iterations of the full one
    again = S.run(s, lams[:1], max_iter=cap)
    assert M.same_bits(again.X[0], got.X[0]).all()
