"""A fixed, seeded stretch of the randomised differential run of every CG solver after fs_cg2 (tools/fuzz_solvers.py is the open-ended
run, recorded in profiles/fuzz_solvers.txt): 40 draws of tests/_truth.make_case per solver, in process, each solved to F twice and
once with a cap, every solve held against the dense longdouble truth and the textbook loop by _truth.check.  A fixed count, not a
time budget: what runs is the same on every machine.  The draws and their truths are made once and shared by all the tests."""
import pytest

import _fuzz_solvers as FZ
import _truth as T
from _gpu import L  # noqa: F401  (the fixture)

SEED, CASES = 20261021, 40
STRETCH = T.stretch(SEED, CASES)
PARAMS = [(s, 0) for s in T.SOLVERS[:5]] + [(s, r) for s in T.SOLVERS[5:] for r in (1, 3, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("solver,ranks", PARAMS, ids=[s if not r else f"{s}-{r}ranks" for s, r in PARAMS])
def test_a_seeded_stretch_is_within_the_bars(L, solver, ranks):  # noqa: F811
    tally = T.Tally()
    for case in STRETCH:
        tally.add(case, solver, FZ.run_and_check(L, case, solver, ranks or None))
    print(tally.line(solver))
    assert tally.cases == CASES and tally.share() >= T.CLASS_FLOOR, tally.line(solver)


@pytest.mark.gpu
def test_the_relations_the_header_states_hold_on_the_stretch(L):  # noqa: F811
    """column j of a panel solver is its single-vector solver under strict_order, pcgn_compact and the two pcgn_kernel forms keep the
    bits, m = 1 and k = 1 fall back to the simpler solver, scheme 0 on virtual ranks is the single-device solver"""
    compared = sum(FZ.relations(L, case) for case in STRETCH)
    strict = sum(c.mode == "strict_order" for c in STRETCH)
    print(f"{compared} pairs of solves compared bit for bit, {strict} of {CASES} draws under strict_order")
    assert strict >= 4 and compared >= 7 * (CASES - sum(c.mode == "cg_fixed_order=0" for c in STRETCH))
