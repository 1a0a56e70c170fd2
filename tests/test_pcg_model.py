"""The CPU model of fs_gram_diag / fs_pcg (tests/_pcg_model.py), pinned on the CPU:

(a) without a preconditioner, from a cold start and with the cap at F it IS the model of fs_cg (tests/_cg_model.py), bit for bit --
    so its formulas and control flow are the pinned ones, and what fs_pcg adds is the only difference;
(b) on the systems a diagonal preconditioner is for (_pcg_model.recipe: 2000 x 300, 8 entries per row, seeds 0-2) against a dense
    numpy.linalg.solve.  Measured with this generator: column-scaled, plain CG ends at the cap of 300 with a true residual of
    2-6 ||b|| (cond 1.7e6-2.3e6), Jacobi converges in 21-22 (preconditioned cond 4.6), true residual 5-10e-9; binary power-law,
    plain 96-112 iterations, Jacobi 19; unscaled control, plain 21-22, Jacobi 18;
(c) warm start, restart from a converged x, the iteration cap, b = 0."""
import os

import numpy as np
import pytest

import _cg_model as M
import _pcg_model as P

SYSTEMS = M.systems()
IDENTITY = [n for n, s in SYSTEMS.items() if np.any(s.b != 0) and s.tol < 1]
SEEDS = (0, 1, 2)


def test_constants_are_the_sources():
    got = M.source_constants()
    assert {k: got.get(k) for k in P.PCG_SOURCE_NAMES} == P.PCG_SOURCE_NAMES
    assert max(P.ST_PCG.values()) < M.CG_STATE_DOUBLES
    at = [v for v in P.ST_PCG.values()]
    assert len(set(at)) == len(at)                       # the new slots collide with none of fs_cg's
    with open(os.path.join(M.ROOT, "include", "fastsparse_hip.h")) as f:
        hdr = " ".join(f.read().split())
    assert "enum { FS_PRECOND_NONE = 0, FS_PRECOND_JACOBI = 1, FS_PRECOND_DIAG = 2 };" in hdr
    assert (P.PRECOND_NONE, P.PRECOND_JACOBI, P.PRECOND_DIAG) == (0, 1, 2)


def test_arithmetic_is_the_sources():
    """the lines of fs_cg.hip the model restates"""
    with open(os.path.join(M.CSRC, "fs_cg.hip")) as f:
        src = " ".join(f.read().split())
    for line in ("const double v = vals ? vals[e] : 1.0; s += v * v;",
                 "for (int e = lo + lane; e < hi; e += 64) {",
                 "if (lane == 0) d[row] = s + lambda;",
                 "dinv[i] = di == 0.0 ? 1.0 : 1.0 / di;",
                 "const double qi = q[i] + lambda * x[i]; q[i] = qi; ri = bi - qi;",
                 "v[0] += bi * bi; v[1] += ri * ri;",
                 "const double stop = arg * sqrt(red[0]);",
                 "st[kStDone] = sqrt(red[1]) <= stop ? 1.0 : 0.0;",
                 "const double zi = PRE ? ri * dinv[i] : ri; p[i] = zi; v[0] += ri * zi;",
                 "const double ri = r[i] - alpha * q[i]; r[i] = ri; const double zi = ri * dinv[i]; v[0] += ri * ri; v[1] += ri * zi;",
                 "const double rr = red[0], rz_new = red[NV - 1];",
                 "else { st[kStBeta] = rz_new / st[kStRsq]; st[kStRsq] = rz_new; st[kStIter] += 1.0; }",
                 "const double zi = r[i] * dinv[i]; p[i] = zi + beta * p[i];"):
        assert line in src, line


def test_gram_diag_is_the_literal_sum():
    """lane by lane: 64 running sums, the butterfly, lambda last -- on rows of 0, 1, 63..65, 130 and 1000 entries"""
    rng = np.random.default_rng(3)
    lens = [0, 1, 63, 64, 65, 130, 1000, 0, 5]
    rp = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    vv = rng.standard_normal(rp[-1]) * np.ldexp(1.0, rng.integers(-20, 20, rp[-1]))
    for vals, lam in ((vv, 0.3), (None, 0.0), (vv, 0.0)):
        want = []
        for j, n in enumerate(lens):
            lane = [0.0] * 64
            for e in range(n):
                v = 1.0 if vals is None else float(vals[rp[j] + e])
                lane[e % 64] += v * v
            m = 32
            while m > 0:
                lane = [lane[l] + lane[l ^ m] for l in range(64)]
                m >>= 1
            want.append(lane[0] + lam)
        got = P.gram_diag((rp, None, vals), lam)
        assert M.same_bits(got, want).all(), (lam, got, want)
        if vals is None:
            assert np.array_equal(got, np.array(lens, float))       # a pattern-only row: its length
    assert np.array_equal(P.dinv_of([0.0, 2.0, -4.0]), [1.0, 0.5, -0.25])


# ---- (a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDENTITY)
def test_without_preconditioner_cold_is_the_cg_model(name):
    s = SYSTEMS[name]
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), s.t_csr_coo())
    want = M.cg(s.ncol, am, atm, s.b, s.lam, s.tol)
    got = P.pcg(s.ncol, am, atm, s.b, s.lam, s.tol, s.ncol, dinv=None, x0=None)
    keys = [k for k in ("alpha", "beta", "rsq", "stop", "done", "iter") if k in want.state]
    assert "alpha" in keys and "rsq" in keys and "stop" in keys
    bad = M.mismatch(got.x, want.x, got.iterations, want.iterations, got.state, {k: want.state[k] for k in keys})
    assert bad is None, (name, bad)
    assert all(k in got.state for k in keys), (name, sorted(got.state))
    again = P.pcg(s.ncol, am, atm, s.b, s.lam, s.tol, 0)             # max_iter <= 0 is F
    assert M.mismatch(again.x, got.x, again.iterations, got.iterations, again.state, got.state) is None, name


# ---- (b) ------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _solved(kind, seed):
    key = (kind, seed)
    if key not in _RUNS:
        s = P.recipe(kind, seed)
        A = P.dense(s)
        K = A.T @ A + s.lam * np.eye(s.ncol)
        res = lambda x: float(np.linalg.norm(K @ x - s.b) / np.linalg.norm(s.b))
        _RUNS[key] = (s, K, res, P.run(s, P.PRECOND_NONE), P.run(s, P.PRECOND_JACOBI))
    return _RUNS[key]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind", ["scaled", "powerlaw", "control"])
def test_jacobi_converges_to_the_dense_solution(kind, seed):
    s, K, res, plain, jac = _solved(kind, seed)
    direct = np.linalg.solve(K, s.b)
    assert res(direct) <= 1e-10                                      # the yardstick itself
    print(f"{s.name}: plain {plain.iterations} (done {plain.state['done']}, residual {res(plain.x):.3g}), "
          f"jacobi {jac.iterations} (residual {res(jac.x):.3g})")
    assert jac.state["done"] == 1.0 and jac.iterations < s.ncol, (s.name, jac.iterations)
    assert res(jac.x) <= 2 * s.tol, (s.name, res(jac.x))
    # ||x - x*|| <= ||K^-1|| ||K x - b|| <= residual ||b|| / lam_min, and lam_min(K) >= lam
    assert np.linalg.norm(jac.x - direct) <= (res(jac.x) + res(direct)) * np.linalg.norm(s.b) / s.lam * 1.01
    if kind == "scaled":
        assert plain.state["done"] == 0.0 and plain.iterations == s.ncol, (s.name, plain.iterations)
        assert res(plain.x) > 1e4 * s.tol, (s.name, res(plain.x))
    elif kind == "powerlaw":
        assert plain.state["done"] == 1.0 and plain.iterations >= 3 * jac.iterations, (s.name, plain.iterations, jac.iterations)
    else:
        assert plain.state["done"] == 1.0 and jac.iterations <= plain.iterations, (s.name, plain.iterations, jac.iterations)


# ---- (c) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_warm_start_restart_and_cap(seed):
    s, K, res, _, cold = _solved("scaled", seed)
    coarse = P.run(s, P.PRECOND_JACOBI, tol=1e-4)
    assert coarse.state["done"] == 1.0 and coarse.iterations < cold.iterations
    warm = P.run(s, P.PRECOND_JACOBI, x0=coarse.x)
    print(f"{s.name}: cold {cold.iterations}, to 1e-4 {coarse.iterations}, then warm {warm.iterations}")
    assert warm.state["done"] == 1.0 and warm.iterations < cold.iterations, (warm.iterations, cold.iterations)
    assert res(warm.x) <= 2 * s.tol
    again = P.run(s, P.PRECOND_JACOBI, x0=cold.x)                    # from a converged x: nothing to do, x keeps its bits
    assert again.iterations == 0 and again.state["done"] == 1.0 and M.same_bits(again.x, cold.x).all()
    assert "alpha" not in again.state
    capped = P.run(s, P.PRECOND_JACOBI, max_iter=5)
    assert capped.iterations == 5 and capped.state["done"] == 0.0
    # the capped solve is the first five iterations of the full one: continuing from it needs no more than the rest plus the
    # restart's loss of conjugacy -- here only that it converges
    assert P.run(s, P.PRECOND_JACOBI, x0=capped.x).state["done"] == 1.0


@pytest.mark.parametrize("precond", [P.PRECOND_NONE, P.PRECOND_JACOBI])
def test_zero_right_hand_side(precond):
    """b = 0: x = 0 and converged, where fs_cg (and bsbm_cg) return NaN"""
    s = SYSTEMS["zero_rhs"]
    assert np.isnan(s.model().x).all()
    r = P.run(s, precond)
    assert r.iterations == 0 and r.state["done"] == 1.0 and r.state["bb"] == 0.0 and r.state["rr"] == 0.0
    assert M.same_bits(r.x, np.zeros(s.ncol)).all()
    # from a warm start the residual is -K x0, not 0: the solve runs (stop = 0: it ends at the cap or on an exact zero)
    w = P.run(s, precond, x0=np.ones(s.ncol), max_iter=3)
    assert w.state["bb"] == 0.0 and w.state["rr"] > 0.0 and w.iterations == 3
