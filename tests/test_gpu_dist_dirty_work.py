"""Sharded solves on work space that has a past (fs_dist_cg, _cg2, _pcg, _pcgn, _pcgn_lambdas, _mscg, _mscgn).

The sharded solvers keep their work space on the handle (ensure_cg_work, ensure_pn_work, ensure_ladder_work, ensure_k of
fs_dist.hip): re-made when k, the scheme or the number of shifts asks for it, otherwise reused as the last solve left it.  The other
suites run well-behaved solves on fresh handles, so what a kept buffer holds before a solve is fresh memory (usually zeros) or finite
numbers of the right size.  Here it is dirt, of three kinds, all made with legal calls:

  poison   freed heap of the per-rank sizes the solve is about to ask for is filled with a tagged NaN (LC.poison_heap:
           fs_device_alloc / fs_device_free) right before a solve that makes, or may re-make, work space: the first solve of a
           handle, a larger k, more shifts, a longer ladder after a shorter one, scheme 0 -> 1 -> 0.  What such a step really
           allocates: the first solve everything; a new k the panels of ensure_pn_work and ensure_k; more shifts or longer vectors
           the ladder's X_i, P_i and scalars (ensure_ladder_work grows, never shrinks: scheme 0 -> 1 keeps them); a scheme change
           the panels of ensure_pn_work, and, like every option change, the k-column vectors of ensure_k.  ensure_cg_work depends on
           F alone, so for fs_dist_cg, _pcg and _mscg the scheme steps run on KEPT vectors: the poison cannot reach those, the two
           kinds below do.  Poison can show a buffer read before it is written ONLY where the allocator hands the poisoned memory back
           (every test asserts that its probes saw some; the count is printed); it cannot show anything about a buffer that is kept.
  nan      a dirtying solve on the same handle, same k and scheme, at least as many shifts, every column of its right-hand side
           holding a NaN, cap 2.  A legal input: FS_OK, every column / pair ends unconverged -- fs_pcg's columns at the cap, fs_mscg's
           pairs where fs_mscg's freeze rule ends a NaN pair (`!(rn > stop)`: at iteration 0; asserted against the model, which is
           what "runs to the cap" comes to for a ladder).  It leaves NaN in R, P, Q, T, the X_i, the P_i, the send slots and the
           gathered sums.  fs_dist_cg / _cg2 have no cap and fs_dist_cg2 refuses NaN norms, so their NaN comes from fs_dist_pcg /
           fs_dist_pcgn (k = 2) solves on the same handle, whose vectors they share.  It cannot show a stale value that only
           meets a NaN-tolerant comparison.
  finite   the same with another system's b scaled by 2^40: a stale finite scalar changes bits where a stale NaN would hide behind
           `!(rn > stop)`.  It cannot show a stale value that is multiplied by an exact zero.
A stray load whose value is discarded is out of scope, as in tests/_lifecycle.py.

Every checked solve runs under strict_order against its model (tests/_dist_*_model.py) bit for bit: X, the infos, rank 0's state
from the debug hooks; nothing is compared with a tolerance.  After every call the caller's B and diag are unchanged, the guards
around X, B and diag are intact (LC.Guarded, in host memory and in HBM), a refused call leaves X with its prefill.  Three virtual
ranks of device 0, and five on a system of three unknowns (empty slices); both dist_cg_scheme values where the solver reads it."""
import contextlib

import numpy as np
import pytest

import _dist_mscgn_model as DN
import _dist_solvers as DV
import _gpu as G
import _lifecycle as LC
import _pcg_model as P
import _pcgn_lambdas_model as NL
import _solvers as SV
from _gpu import FS_ERR_ARG, FS_ERR_NO_TRANSPOSE, FS_ERR_RELEASED, FS_OK, L  # noqa: F401

pytestmark = pytest.mark.gpu

SYSTEMS = (("fixture_100x50", 3), ("binary_F65", 3), ("binary_F257", 3), ("control_seed0", 3), ("three_eigenvalues", 5))
K = 5                                                                 # columns of the k-column solvers (odd: slices of odd length)
DIRTY_CAP = 2
COUNTS = {}                                                           # (solver, kind of dirt) -> checked solves
POISON = {"seen": 0, "probed": 0}


def _schemes(solver, ranks):
    return (0, 1) if solver in DV.READS_SCHEME and ranks > 1 else (0,)


def _two(s):
    i = np.arange(s.ncol, dtype=np.float64)
    return np.ascontiguousarray(np.stack([s.b, s.b * 1.5 + np.sin(i * 0.22 + 0.6)], 1))


def checked_cases(solver, s, k=K):
    """(name, arguments of DirtyFrame.solve / .check): a cold solve, a warm one where the solver has one, a right-hand side with a
    zero column (SV.columns: column 2, frozen at the start; column 1 duplicates column 0), B = 0 with tol >= 1 (no product is
    enqueued), fewer shifts than the dirtying solve's eight.  Caps of at most 12 where F > 50: the models are Python.
    fs_dist_cg2 has the cold solve alone: it has no warm start, no look before its first iteration and divides by the norms of B's
    columns, so B = 0 or a zero column is 0 / 0 in every entry of X from the first line on (the reference's behaviour, kept: the
    systems cg2_zero_column and cg2_equal_columns of the solver suites), which would compare NaN with NaN whatever the work space held"""
    F = s.ncol
    cap = 0 if F <= 50 else 12
    B = SV.columns(s, k)
    dg = SV.caller_diag(s)
    if solver == "cg":
        # (b = 0: fs_dist_cg takes no look before its first iteration -- 0 / 0, NaN for F iterations, as the header says)
        return [("cold", dict(B=s.b, tol=s.tol if F <= 65 else 1e-3)), ("b = 0, tol 1", dict(B=np.zeros(F), tol=1.0))]
    if solver == "cg2":
        return [("cold", dict(B=_two(s), tol=s.tol if F <= 65 else 1e-3))]
    if solver == "pcg":
        return [("cold jacobi", dict(B=s.b, precond=P.PRECOND_JACOBI, cap=cap)), ("warm", dict(B=s.b, X0=SV.x0(s), cap=cap)),
                ("warm diag cap 3", dict(B=s.b, X0=SV.x0(s), precond=P.PRECOND_DIAG, diag=dg, cap=3)),
                ("b = 0, tol 1", dict(B=np.zeros(F), tol=1.0, precond=P.PRECOND_JACOBI))]
    if solver in ("pcgn", "pcgn_lambdas"):
        lams = dict(lams=NL.rungs(s, k)) if solver == "pcgn_lambdas" else {}
        return [("cold jacobi, a zero column", dict(B=B, precond=P.PRECOND_JACOBI, cap=cap, **lams)),
                ("warm", dict(B=B, X0=SV.x0_columns(s, B), cap=cap, **lams)),
                ("warm diag cap 3", dict(B=B, X0=SV.x0_columns(s, B), precond=P.PRECOND_DIAG, diag=dg, cap=3, **lams)),
                ("B = 0, tol 1", dict(B=np.zeros((F, k)), tol=1.0, precond=P.PRECOND_JACOBI, **lams))]
    b = s.b if solver == "mscg" else B
    zero = np.zeros(F) if solver == "mscg" else np.zeros((F, k))
    return [("cold, the ladder of 8", dict(B=b, lams=SV.lams_of(s, "m8"), cap=cap, pad=3)),
            ("three shifts, the smallest twice", dict(B=b, lams=SV.lams_of(s, "m3"), cap=cap or 5)),
            ("one shift", dict(B=b, lams=SV.lams_of(s, "m1"), cap=cap, pad=3)),
            ("B = 0, tol 1, three shifts", dict(B=zero, lams=SV.lams_of(s, "m3"), tol=1.0))]


def _garbage(s, k, kind):
    """the right-hand side of a dirtying solve: every column holds a NaN, or is another system's b scaled by 2^40"""
    F = s.ncol
    if kind == "nan":
        B = SV.columns(s, max(k, 3))[:, :k].copy()
        B[:, 2:3] = s.b[:, None] * 0.5                                # (no zero column: every column holds a NaN)
        B[7 % F, :] = np.nan
    else:
        other = SV.ALL["fixture_100x50" if s.name != "fixture_100x50" else "binary_F65"].b
        B = np.stack([np.resize(other, F) * (1.0 + 0.25 * j) * 2.0 ** 40 + j for j in range(k)], 1)
    return np.ascontiguousarray(B)


def dirty(fr, solver, kind, scheme, k=K):
    """the dirtying solves for `solver` on fr's handle; returns how many ran"""
    s = fr.s
    lams8 = SV.lams_of(s, "m8")
    kk = 2 if solver == "cg2" else k if solver in DV.K_COLUMN else 1
    B = _garbage(s, kk, kind)
    b1 = np.ascontiguousarray(B[:, 0])
    runs = []
    if solver in ("cg", "cg2") and kind == "finite":                  # (no cap: a tol the garbage meets soon)
        runs.append((solver, dict(B=b1 if solver == "cg" else B, tol=1e-2)))
    elif solver == "cg":
        runs.append(("pcg", dict(B=b1, precond=P.PRECOND_JACOBI)))
        runs.append(("mscg", dict(B=b1, lams=lams8)))
    elif solver == "cg2":
        runs.append(("pcgn", dict(B=B, precond=P.PRECOND_JACOBI)))
    elif solver in DV.PCG_FAMILY:
        lams = dict(lams=NL.rungs(s, kk)) if solver == "pcgn_lambdas" else {}
        runs.append((solver, dict(B=b1 if solver == "pcg" else B, precond=P.PRECOND_JACOBI, **lams)))
    else:
        runs.append((solver, dict(B=b1 if solver == "mscg" else B, lams=lams8)))
        runs.append(("pcg", dict(B=b1, precond=P.PRECOND_JACOBI)) if solver == "mscg" else
                    ("pcgn_lambdas", dict(B=B, lams=NL.rungs(s, kk), precond=P.PRECOND_JACOBI)))
    for sv, kw in runs:
        kw.setdefault("cap", DIRTY_CAP)
        rc, X, infos = fr.solve(sv, hbm=bool(fr.solves & 2), **kw)
        what = (s.name, solver, kind, scheme, "the dirtying solve", sv)
        assert rc == FS_OK, (what, rc, fr.L.fs_last_error())
        if kind != "nan" or sv in ("cg", "cg2"):
            continue
        assert np.isnan(X).any(), what
        flat = [i for row in infos for i in row] if sv == "mscgn" else infos
        assert all(i.converged == 0 for i in flat), (what, [i.converged for i in flat])
        if sv in DV.PCG_FAMILY:
            assert all(i.iterations == DIRTY_CAP for i in flat), (what, [i.iterations for i in flat])
        else:                                                        # fs_mscg's freeze rule on a NaN pair: the model's count
            Bc = kw["B"].reshape(s.ncol, -1)
            bounds = fr.bounds if scheme == 1 and fr.dist.ranks > 1 else None
            for j in range(Bc.shape[1]):
                col = fr.column("mscg", np.ascontiguousarray(Bc[:, j]), 0.0, kw["lams"], s.tol, kw["cap"], None, None, bounds)
                mine = [row[j] for row in infos] if sv == "mscgn" else infos
                assert [i.iterations for i in mine] == [i.iterations for i in col.infos], (what, j)
    return len(runs)


def run_checked(fr, solver, kind, scheme, cases):
    for n, (name, kw) in enumerate(cases):
        what = f"fs_dist_{solver} {name} on {fr.s.name}, {fr.dist.ranks} ranks, scheme {scheme}, after {kind}"
        rc, X, infos = fr.solve(solver, hbm=bool(n & 1), **kw)
        assert rc == FS_OK, (what, rc, fr.L.fs_last_error())
        fr.check(what, solver, scheme, X, infos, **{a: v for a, v in kw.items() if a != "pad"})
        COUNTS[(solver, kind)] = COUNTS.get((solver, kind), 0) + 1


@contextlib.contextmanager
def frame(L, name, ranks, pair_bounds=None):
    s = SV.ALL[name]
    dist = DV.CutPair(L, s, pair_bounds) if pair_bounds else DV.Dist(L, s, ranks, False)
    try:
        t_csr = dist.t_csr() if pair_bounds else DV.sorted_t(dist, s)
        yield DV.DirtyFrame(L, dist, s, t_csr, dist.bounds_t(), kmax=K)
    finally:
        dist.close()


# ---- 1: poison ---------------------------------------------------------------------------------------------------------------
def _poison(fr, solver, scheme, k, m, lams):
    s = fr.s
    nslots = 0 if lams is None else len([v for v in lams if v != min(lams)])
    seen, probed = LC.poison_heap(fr.L, DV.work_space_per_rank(solver, s.ncol, s.nrow, fr.bounds, k, m, nslots, scheme))
    POISON["seen"] += seen
    POISON["probed"] += probed


@pytest.mark.parametrize("solver", DV.SOLVERS)
def test_work_space_made_from_poisoned_heap(L, solver):
    """a fresh handle: poison, then the first solve; poison again before every solve that asks for other work space -- a larger k,
    more shifts (a longer ladder after a shorter one), scheme 0 to 1 and back (which of these steps allocate: the module's text)"""
    seen0 = POISON["seen"]
    for name, ranks in SYSTEMS:
        with frame(L, name, ranks) as fr:
            s = fr.s
            full = checked_cases(solver, s)
            small = checked_cases(solver, s, 3) if solver in ("pcgn", "pcgn_lambdas", "mscgn") else full
            # (scheme, cases): the work space grows from step to step
            if solver in DV.LADDER:
                steps = [(0, small[2:3]), (0, small[1:2]), (0, full[0:1]), (1, full[1:2]), (1, full[0:1]), (0, full[0:1])]
            elif solver in ("pcgn", "pcgn_lambdas"):
                steps = [(0, small[0:1]), (0, full[1:2]), (1, full[0:1]), (0, full[2:3])]
            else:
                steps = [(0, full[0:1]), (1, full[1:2] or full[0:1]), (0, full[0:1])]
            for scheme, cases in steps:
                if scheme not in _schemes(solver, ranks) and solver not in ("cg2", "pcgn"):
                    continue
                with G.options(strict_order=1, dist_cg_scheme=scheme):
                    kw = cases[0][1]
                    B = kw["B"]
                    _poison(fr, solver, scheme, B.shape[1] if B.ndim == 2 else 1, len(kw.get("lams") or [0]) if solver in DV.LADDER else 1,
                            kw.get("lams") if solver in DV.LADDER else None)
                    run_checked(fr, solver, "poison", scheme, cases)
    print(f"poison probes so far: {POISON['seen']} of {POISON['probed']} doubles still held the poison")
    assert POISON["seen"] > seen0, (solver, "no probe of this test saw its poison again: these solves showed nothing")


# ---- 2, 3: NaN and finite garbage through the API ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("nan", "finite"))
@pytest.mark.parametrize("solver", DV.SOLVERS)
def test_kept_work_space_dirtied_through_the_api(L, solver, kind):
    """the dirtying solve(s), then at once every checked solve of the solver, each again right behind a dirtying solve; then the
    resident products on the vectors the solvers clobber"""
    for name, ranks in SYSTEMS:
        with frame(L, name, ranks) as fr:
            cases = checked_cases(solver, fr.s)
            for scheme in _schemes(solver, ranks):
                with G.options(strict_order=1, dist_cg_scheme=scheme):
                    for case in cases:
                        dirty(fr, solver, kind, scheme)
                        run_checked(fr, solver, kind, scheme, [case])
                    dirty(fr, solver, kind, scheme)
                    run_checked(fr, solver, kind, scheme, cases)     # (and one behind the other, on what the checked solves leave)
                    dirty(fr, solver, kind, scheme)
                    fr.resident_products_exact((name, solver, kind, scheme))


# ---- pair handles ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ("pcgn_lambdas", "mscgn"))
def test_pair_handle_on_the_cuts_that_tell_the_schemes_apart(L, solver):
    """fs_dist_matrix_pair with A' in the caller's entry order, cut at _dist_mscgn_model.DIFFERING_BOUNDS: all three kinds of dirt"""
    name = "control_seed0"
    with frame(L, name, 3, pair_bounds=DN.DIFFERING_BOUNDS[name]) as fr:
        assert fr.bounds == DN.DIFFERING_BOUNDS[name], fr.bounds
        cases = checked_cases(solver, fr.s)
        for scheme in (0, 1):
            with G.options(strict_order=1, dist_cg_scheme=scheme):
                kw = cases[0][1]
                _poison(fr, solver, scheme, K, len(kw["lams"]) if solver in DV.LADDER else 1, kw.get("lams") if solver in DV.LADDER else None)
                run_checked(fr, solver, "poison", scheme, cases[:1])
                for kind in ("nan", "finite"):
                    dirty(fr, solver, kind, scheme)
                    run_checked(fr, solver, kind, scheme, cases)


# ---- refused calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", DV.SOLVERS)
def test_a_refused_call_right_after_a_dirtying_solve_leaves_x_alone(L, solver):
    """FS_ERR_ARG, FS_ERR_NO_TRANSPOSE and (a shard of A' that gave its plain CSR back, under strict_order) FS_ERR_RELEASED, each
    right behind a dirtying solve: X keeps its prefill (DirtyFrame.solve asserts it), and the solve after it has the model's bits"""
    name, ranks = "control_seed0", 3
    s = SV.ALL[name]
    with contextlib.ExitStack() as stack:
        with G.options(binning=2, bin_flags=64):                       # kept two-pass copies: there is something to release for
            fr = stack.enter_context(frame(L, name, ranks))
        M_not = stack.enter_context(DV.handle_without_transpose(L, fr.dist, s))
        cases = checked_cases(solver, s)
        kw0 = cases[0][1]
        bad = dict(B=0) if solver in ("cg", "cg2") else dict(tol=-1e-8)          # (fs_dist_cg checks nothing but its pointers)
        for scheme in _schemes(solver, ranks):
            with G.options(strict_order=1, dist_cg_scheme=scheme):
                for kind in ("nan", "finite"):
                    for raw, want in ((bad, FS_ERR_ARG), (dict(M=M_not), FS_ERR_NO_TRANSPOSE)):
                        dirty(fr, solver, kind, scheme)
                        rc, _, _ = fr.solve(solver, raw=raw, hbm=kind == "nan", **kw0)
                        assert rc == want, (solver, scheme, kind, raw, rc)
                    run_checked(fr, solver, kind, scheme, cases[:1])
        for scheme in _schemes(solver, ranks):                         # the last dirt before the release
            with G.options(strict_order=1, dist_cg_scheme=scheme):
                dirty(fr, solver, "finite", scheme)
        assert L.fs_matrix_release_csr(L.fs_dist_matrix_shard(fr.dist.M, 1, 1)) == 1
        for scheme in _schemes(solver, ranks)[::-1]:
            with G.options(strict_order=1, dist_cg_scheme=scheme):
                rc, _, _ = fr.solve(solver, hbm=True, **kw0)
                assert rc == FS_ERR_RELEASED, (solver, scheme, rc, L.fs_last_error())


# checked solves per solver, as the loops above make them: (after poison, after NaN, after finite garbage)
EXPECTED = {"cg": (15, 42, 42), "cg2": (15, 11, 11), "pcg": (15, 82, 82), "pcgn": (20, 41, 41), "pcgn_lambdas": (22, 90, 90),
            "mscg": (30, 82, 82), "mscgn": (32, 90, 90)}


def test_the_counts():
    """last in the file, and about the whole file: what ran on which dirt is what the parametrisation is meant to run, no case
    lost; and the allocator handed at least a tenth of the probed doubles back with their poison"""
    assert COUNTS, "this test counts what the tests above ran: run the whole file"
    for i, kind in enumerate(("poison", "nan", "finite")):
        print(f"checked solves after {kind}: " + ", ".join(f"fs_dist_{sv} {COUNTS.get((sv, kind), 0)}" for sv in DV.SOLVERS))
    print(f"poison probes: {POISON['seen']} of {POISON['probed']} doubles still held the poison")
    got = {sv: tuple(COUNTS.get((sv, kind), 0) for kind in ("poison", "nan", "finite")) for sv in DV.SOLVERS}
    assert got == EXPECTED, got
    assert POISON["probed"] > 0 and 10 * POISON["seen"] >= POISON["probed"], POISON
