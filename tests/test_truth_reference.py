"""tests/_truth.py on the CPU: the project's models go through check() as if they were the device and must all pass (so the bars
are reachable before anything runs on a GPU); ten hand-made faults must each be caught by the check named for it; and the reference
reproduces the exactly solvable family."""
import numpy as np
import pytest

import _cg_model as M
import _dist_mscg_model as DS
import _dist_pcg_model as DP
import _mscg_model as S
import _pcg_model as P
import _truth as T

SEED, CASES = 20261021, 60
STRETCH = T.stretch(SEED, CASES)


# ---- the device's first stage, without its zeros -----------------------------------------------------------------------------
def _stage1_short(terms):
    """_cg_model.stage1 for at most kRedBlocks kRedThreads terms: thread (b, t) holds 0.0 + terms[256 b + t] or +0.0, so only the first
    ceil(n / 256) blocks have anything to add.  The models call stage1 three times per iteration and column on 262144 padded terms;
    the stretches here have F <= 513"""
    terms = np.asarray(terms, np.float64).reshape(-1)
    if terms.size > M.RED_BLOCKS * M.RED_THREADS:
        return _STAGE1(terms)
    nb = -(-terms.size // M.RED_THREADS)
    pad = np.zeros(nb * M.RED_THREADS)
    pad[:terms.size] = terms
    out = np.zeros(M.RED_BLOCKS)
    out[:nb] = M._block_sum((np.zeros(pad.size) + pad).reshape(nb, M.RED_THREADS))
    return out


_STAGE1 = M.stage1


@pytest.fixture(autouse=True)
def short_stage1(monkeypatch):
    monkeypatch.setattr(M, "stage1", _stage1_short)


def test_the_short_first_stage_has_the_models_bits():
    rng = np.random.default_rng(3)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 513, 1000):
        v = rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-30, 30, n))
        v[::7] = -0.0
        assert M.same_bits(_stage1_short(v), _STAGE1(v)).all(), n


# ---- the models as a backend -----------------------------------------------------------------------------------------------
_PRODUCTS = {}


def products(case):
    key = (case.seed, case.draw)
    if key not in _PRODUCTS:
        s = M.System(f"draw{case.draw}", case.nrow, case.F, case.rows, case.cols, case.vals, case.B[:, 0], None, case.lam, case.tol)
        t_csr = s.t_csr_coo()
        am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr)
        _PRODUCTS[key] = (t_csr, am, atm)
    return _PRODUCTS[key]


def three_slices(F):
    """the row cuts of A' on three ranks (F < 3 leaves slices empty)"""
    return [0, F // 3, (2 * F) // 3, F]


def model_solve(case, solver, cap, tol, tree, lams=None, x_from_zero=False):
    """X (m, F, k) and the m k infos of the project's model of `solver`: P.pcg per column (fs_pcg, fs_pcgn, fs_pcgn_lambdas), S.mscg
    per column (fs_mscg, fs_mscgn); the sharded solvers with the slice reducer on three slices"""
    t_csr, am, atm = products(case)
    m, k = case.shape(solver)
    F, B = case.F, case.B_of(solver)
    lams = case.lams(solver) if lams is None else lams
    dist = solver.startswith("dist_")
    bounds = three_slices(F) if dist else None
    X, infos = np.zeros((m, F, k)), [None] * (m * k)
    X0 = case.X0(solver)
    for j in range(k):
        if T.preconditioned(solver):
            lam = float(lams[0, j])
            dinv = None
            if case.precond == T.JACOBI:
                dinv = P.dinv_of(P.gram_diag(t_csr, lam))
            elif case.precond == T.DIAG:
                dinv = P.dinv_of(case.diag)
            x0 = None if X0 is None else X0[:, j]
            col = (DP.pcg(F, am, atm, B[:, j], lam, tol, cap, dinv, x0, bounds) if dist else
                   P.pcg(F, am, atm, B[:, j], lam, tol, cap, dinv, x0, tree))
            X[0, :, j] = col.x - (x0 if x_from_zero and x0 is not None else 0.0)
            with np.errstate(all="ignore"):
                infos[j] = T.Info(col.iterations, int(col.state["done"]), float(np.sqrt(col.state["rr"])), float(np.sqrt(col.state["bb"])))
        else:
            col = (DS.mscg(F, am, atm, B[:, j], lams[:, j], tol, cap, bounds) if dist else S.mscg(F, am, atm, B[:, j], lams[:, j], tol, cap, tree))
            X[:, :, j] = col.X
            for i in range(m):
                g = col.infos[i]
                infos[i * k + j] = T.Info(int(g.iterations), int(g.converged), float(g.rnorm), float(g.bnorm))
    return X, infos


def as_result(case, solver, cap, tol, X, infos, again=True):
    m, k = case.shape(solver)
    xoff, ldx, _, _, _ = case.layout(solver)
    xbuf, bbuf = case.buffers(solver)
    for i in range(m):
        xbuf[xoff + i * ldx:xoff + i * ldx + case.F * k] = X[i].reshape(-1)
    return T.Result(solver, cap, tol, T.FS_OK, xbuf, bbuf, list(infos), (xbuf.copy(), list(infos)) if again else None)


# ---- no false alarms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,tree", [(s, t) for s in T.SOLVERS[:5] for t in ("serial", "device")] + [(s, "device") for s in T.SOLVERS[5:]])
def test_every_model_passes_the_checks(solver, tree):
    tally = T.Tally()
    for case in STRETCH:
        outs = []
        for cap, tol in case.solves():
            X, infos = model_solve(case, solver, cap, tol, tree)
            outs.append(T.check(case, as_result(case, solver, cap, tol, X, infos)))
        tally.add(case, solver, outs)
    print(tally.line(solver))
    assert tally.share() >= T.CLASS_FLOOR, tally.line(solver)
    assert {c.mode for c in STRETCH} == set(T.MODES)


def test_the_stretches_keep_the_class_floor():
    """the floor of 60 % per solver, on the stretch of tests/test_gpu_fuzz_solvers.py as well (drawn the same way, full sizes)"""
    for cases in (STRETCH, T.stretch(SEED + 1, 300)):
        for solver in T.SOLVERS:
            share = sum(c.in_class(solver) for c in cases) / len(cases)
            print(f"{solver}: {100 * share:.0f} % of {len(cases)} cases in the count class")
            assert share >= T.CLASS_FLOOR, (solver, share)


# ---- teeth -----------------------------------------------------------------------------------------------------------------
def caught(solver, fault, wanted):
    """the names of the checks that `fault(case, solver, cap, tol)` -> Result or None (not applicable) fails on the stretch, split by
    (full solves, capped solves); stops at the first case that fails with `wanted`"""
    names = (set(), set())
    for case in STRETCH:
        for n, (cap, tol) in enumerate(case.solves()):
            result = fault(case, solver, cap, tol)
            if result is None:
                continue
            try:
                T.check(case, result)
            except T.CheckFailed as e:
                names[n].add(e.name)
        if wanted in names[0] | names[1]:
            break
    return names


def _plain(case, solver, cap, tol, **kw):
    return model_solve(case, solver, cap, tol, "serial", **kw)


def fault_next_lambda(case, solver, cap, tol):
    if case.k < 2 or len(set(case.lams_k)) < 2:
        return None
    X, infos = _plain(case, solver, cap, tol, lams=np.roll(case.lams(solver), -1, axis=1))
    return as_result(case, solver, cap, tol, X, infos)


def fault_sigma_from_first(case, solver, cap, tol):
    """sigma_i = lambda[i] - lambda[0] on a sequence that runs at the minimum: x_i solves at min + lambda[i] - lambda[0]"""
    lams = case.lams(solver)
    if lams[0, 0] == lams.min():
        return None
    wrong = np.maximum(lams.min() + lams - lams[0:1], lams.min() * 1e-3)
    X, infos = _plain(case, solver, cap, tol, lams=wrong)
    return as_result(case, solver, cap, tol, X, infos)


def fault_early_freeze(case, solver, cap, tol):
    """freezes at 10 stop and says converged (its rnorm reported as a converged column's would be)"""
    if tol == 0:
        return None
    X, infos = _plain(case, solver, cap, 10 * tol)
    return as_result(case, solver, cap, tol, X, [g._replace(rnorm=g.rnorm / 10) if g.converged else g for g in infos])


def fault_swapped_columns(case, solver, cap, tol):
    if case.k < 2:
        return None
    X, infos = _plain(case, solver, cap, tol)
    X[:, :, [0, 1]] = X[:, :, [1, 0]]
    return as_result(case, solver, cap, tol, X, infos)


def fault_counts_three_high(case, solver, cap, tol):
    X, infos = _plain(case, solver, cap, tol)
    return as_result(case, solver, cap, tol, X, [g._replace(iterations=g.iterations + 3) for g in infos])


def fault_warm_x_from_zero(case, solver, cap, tol):
    if not case.warm(solver):
        return None
    X, infos = _plain(case, solver, cap, tol, x_from_zero=True)
    return as_result(case, solver, cap, tol, X, infos)


def fault_steps_away(case, solver, cap, tol):
    """(not one of the ten: check 5's first half alone) every update of x has the wrong sign"""
    X, infos = _plain(case, solver, cap, tol)
    return as_result(case, solver, cap, tol, -X, infos)


def fault_last_row_stale(case, solver, cap, tol):
    X, infos = _plain(case, solver, cap, tol)
    X0 = case.X0(solver)
    j = X.shape[2] - 1
    X[:, -1, j] = 0.0 if X0 is None else X0[-1, j]
    return as_result(case, solver, cap, tol, X, infos)


def fault_neighbours_bnorm(case, solver, cap, tol):
    if case.k < 2:
        return None
    X, infos = _plain(case, solver, cap, tol)
    k = case.shape(solver)[1]
    return as_result(case, solver, cap, tol, X, [g._replace(bnorm=infos[(n // k) * k + (n % k + 1) % k].bnorm) for n, g in enumerate(infos)])


def fault_minus_zero(case, solver, cap, tol):
    X, infos = _plain(case, solver, cap, tol)
    zero = ~case.B_of(solver).any(0)
    if not zero.any():
        return None
    X[:, :, zero] = -0.0
    return as_result(case, solver, cap, tol, X, infos)


def fault_second_run_one_bit(case, solver, cap, tol):
    X, infos = _plain(case, solver, cap, tol)
    r = as_result(case, solver, cap, tol, X, infos)
    xoff = case.layout(solver)[0]
    r.again[0].view(np.int64)[xoff] ^= 1
    return r


# (the fault, the solver it is handed to, the solve -- 0: run to F, 1: capped -- and the check that must catch it there)
TEETH = [(fault_next_lambda, "pcgn_lambdas", 0, "true residual"),
         (fault_sigma_from_first, "mscg", 0, "true residual"), (fault_sigma_from_first, "mscgn", 0, "true residual"),
         (fault_early_freeze, "pcgn", 0, "true residual"),
         (fault_swapped_columns, "pcgn", 0, "true residual"), (fault_swapped_columns, "mscgn", 0, "true residual"),
         (fault_counts_three_high, "pcg", 0, "iteration count"), (fault_counts_three_high, "mscgn", 0, "iteration count"),
         (fault_warm_x_from_zero, "pcgn_lambdas", 0, "true residual"), (fault_steps_away, "mscg", 1, "energy norm"),
         (fault_last_row_stale, "pcgn", 0, "true residual"), (fault_last_row_stale, "mscgn", 1, "capped iterate"),
         (fault_neighbours_bnorm, "pcgn", 0, "info"), (fault_neighbours_bnorm, "mscgn", 0, "info"),
         (fault_minus_zero, "pcgn", 0, "frozen"), (fault_minus_zero, "mscg", 0, "frozen"),
         (fault_second_run_one_bit, "pcg", 0, "repeat"), (fault_second_run_one_bit, "mscgn", 0, "repeat")]


@pytest.mark.parametrize("fault,solver,solve,name", TEETH, ids=[f"{f.__name__[6:]}-{s}-{n.replace(' ', '_')}" for f, s, _, n in TEETH])
def test_a_fault_is_caught_by_the_check_named_for_it(fault, solver, solve, name):
    names = caught(solver, fault, name)
    assert name in names[solve], (fault.__name__, solver, "full" if solve == 0 else "capped", names)


def test_a_twin_with_other_bits_is_caught():
    """check 7's other half: a duplicate column that differs from its twin in one bit"""
    hits = 0
    for case in STRETCH:
        if not case.twins("pcgn") or case.mode == "cg_fixed_order=0":
            continue
        cap, tol = case.solves()[0]
        X, infos = _plain(case, "pcgn", cap, tol)
        j = case.twins("pcgn")[0][0]
        X[0, :, j].view(np.int64)[0] ^= 1
        with pytest.raises(T.CheckFailed) as e:
            T.check(case, as_result(case, "pcgn", cap, tol, X, infos))
        assert e.value.name in ("twins", "true residual", "frozen"), e.value
        hits += e.value.name == "twins"
    assert hits >= 1


# ---- the reference itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("valued", [False, True])
def test_the_reference_is_exact_on_the_exact_family(valued):
    """A'A = d I with d + lam = c a power of two and dyadic b: x = b / c exactly; the textbook loop is done after one pass (count 0,
    converged), and at once from x0 = b / c"""
    fam = M.exact_family(valued, F=400)
    s = fam.s
    c = T.Case()
    c.nrow, c.F, c.rows, c.cols, c.vals, c.B = s.nrow, s.ncol, s.rows, s.cols, s.vals, fam.panel(4)
    t = T.dense_truth(c)
    assert np.array_equal(t.K.astype(np.float64), np.eye(s.ncol) * fam.d)
    live = [j for j in range(4) if c.B[:, j].any()]
    xs = t.xstar([s.lam] * len(live), live)
    assert np.array_equal(xs.astype(np.float64), c.B[:, live] / fam.c) and np.array_equal(xs, (c.B[:, live] / fam.c).astype(T.LD))
    for j in live:
        for d in (None, t.gram + s.lam, fam.diag):
            for ref in T.textbook_pcg(t.K, c.B[:, j], s.lam, 1e-6, 0, d):
                assert (ref.iterations, ref.converged) == (0, 1) and np.array_equal(np.asarray(ref.x, np.float64), c.B[:, j] / fam.c), (j, ref)
                assert ref.rnorm == 0
            for ref in T.textbook_pcg(t.K, c.B[:, j], s.lam, 1e-6, 0, d, x0=c.B[:, j] / fam.c):
                assert (ref.iterations, ref.converged, ref.rnorm) == (0, 1, 0), (j, ref)
            one = T.textbook_loop(t.K, c.B[:, j], s.lam, 1e-6, 0, d, fam.x0(c.B, "other")[:, j])
            assert (one.iterations, one.converged) == (0, 1) and np.array_equal(np.asarray(one.x, np.float64), c.B[:, j] / fam.c)
    zero = T.textbook_loop(t.K, np.zeros(s.ncol), s.lam, 1e-6, 0)
    assert (zero.iterations, zero.converged) == (0, 1) and not zero.x.any()


def test_the_capped_bar_is_what_the_textbook_loops_measure():
    """check 5's bar is 100 times the worst relative deviation of the float64 textbook loops from the longdouble one at the capped
    iterate, over the count class of the stretch tests/test_gpu_fuzz_solvers.py runs: the recorded figure is not exceeded"""
    worst = T.measure_capped(T.stretch(SEED, 40))
    print(f"worst relative deviation of a float64 textbook loop from the longdouble one at a capped iterate: {worst:.3g}; "
          f"recorded {T.CAPPED_MEASURED:.3g}; the bar {T.CAPPED_BAR:.3g}")
    assert worst <= T.CAPPED_MEASURED
