"""The CPU model of fs_dist_pcg (tests/_dist_pcg_model.py), pinned on the CPU:

(a) with bounds=None (scheme 0, and scheme 1 on one rank) it IS the model of fs_pcg, bit for bit: every recipe and seed, without a
    preconditioner, with Jacobi and with a caller's diagonal, warm and capped;
(b) with bounds whose only non-empty slice is the whole vector it still is: an empty slice contributes +0.0, and stage 2 over
    {+0.0, s, +0.0} is s;
(c) with three non-empty slices the slice tree rounds differently: on each of the three seed-0 recipes at least one entry of x
    differs in its bits from the whole-vector model (which is what lets the GPU test tell scheme 1 from scheme 0);
(d) the launchers and scalar steps the model names exist in the sources, and the state slots are fs_pcg's."""
import os
import re

import numpy as np
import pytest

import _cg_model as M
import _dist_pcg_model as DP
import _pcg_model as P
from _solvers import caller_diag as _caller_diag, x0 as _x0

KINDS = ("scaled", "powerlaw", "control")
SEEDS = (0, 1, 2)
# (case, precond, warm start, max_iter): plain CG is capped here, it needs 100-300 iterations on these systems
CASES = [("none-cap12", P.PRECOND_NONE, False, 12), ("jacobi", P.PRECOND_JACOBI, False, 0), ("diag", P.PRECOND_DIAG, False, 0),
         ("jacobi-warm", P.PRECOND_JACOBI, True, 0), ("none-warm-cap7", P.PRECOND_NONE, True, 7), ("jacobi-cap5", P.PRECOND_JACOBI, False, 5),
         ("diag-warm-cap3", P.PRECOND_DIAG, True, 3)]
_RECIPES = {}


def _recipe(kind, seed):
    if (kind, seed) not in _RECIPES:
        _RECIPES[(kind, seed)] = P.recipe(kind, seed)
    return _RECIPES[(kind, seed)]


def _pair(s, case, bounds):
    _, precond, warm, max_iter = case
    kw = dict(max_iter=max_iter, x0=_x0(s) if warm else None, diag=_caller_diag(s) if precond == P.PRECOND_DIAG else None)
    return P.run(s, precond, **kw), DP.run(s, precond, bounds=bounds, **kw)


def _same(want, got):
    assert set(got.state) == set(want.state), (sorted(got.state), sorted(want.state))
    return M.mismatch(got.x, want.x, got.iterations, want.iterations, got.state, want.state)


# ---- (a), (b) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind", KINDS)
def test_without_bounds_and_with_empty_slices_it_is_the_pcg_model(kind, seed):
    s = _recipe(kind, seed)
    for case in CASES:
        want, got = _pair(s, case, None)
        assert _same(want, got) is None, (s.name, case[0], _same(want, got))
    F = s.ncol
    more = ((CASES[6], [0, 0, F, F]), (CASES[3], [0, 0, 0, 0, F])) if seed == 0 else ()
    for case, bounds in ((CASES[1], [0, 0, F, F]),) + more:
        want, got = _pair(s, case, bounds)
        assert _same(want, got) is None, (s.name, case[0], bounds, _same(want, got))


def test_an_empty_slice_is_plus_zero():
    assert M.stage2(M.stage1(np.zeros(0))) == 0.0 and not np.signbit(M.stage2(M.stage1(np.zeros(0))))
    v = np.random.default_rng(5).standard_normal(300)
    whole = M.Reducer("device")(v)
    assert M.same_bits(M.Reducer("device", [0, 0, 300, 300])(v), whole)[0]
    assert M.same_bits(M.Reducer("device", [0, 300, 300, 300, 300, 300])(v), whole)[0]


def test_zero_rhs_and_restart_from_a_converged_x():
    s = M.systems(large=False)["zero_rhs"]
    for bounds in (None, [0, 20, 41, 64]):
        for precond in (P.PRECOND_NONE, P.PRECOND_JACOBI):
            r = DP.run(s, precond, bounds=bounds)
            assert r.iterations == 0 and r.state["done"] == 1.0 and r.state["bb"] == 0.0 and M.same_bits(r.x, np.zeros(s.ncol)).all()
    s = _recipe("scaled", 0)
    bounds = DP.DIFFERING_BOUNDS[s.name]
    cold = DP.run(s, P.PRECOND_JACOBI, bounds=bounds)
    again = DP.run(s, P.PRECOND_JACOBI, x0=cold.x, bounds=bounds)
    assert cold.state["done"] == 1.0 and again.iterations == 0 and again.state["done"] == 1.0 and M.same_bits(again.x, cold.x).all()
    assert "alpha" not in again.state


# ---- (c) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DP.DIFFERING_BOUNDS))
def test_three_slices_round_differently(name):
    s = _recipe(name.split("_")[0], 0)
    bounds = DP.DIFFERING_BOUNDS[name]
    assert bounds[0] == 0 and bounds[-1] == s.ncol and all(a < b for a, b in zip(bounds, bounds[1:]))
    want, got = _pair(s, CASES[1], bounds)
    differ = int((~M.same_bits(got.x, want.x)).sum())
    print(f"{name} bounds {bounds}: {differ} of {s.ncol} entries of x differ in their bits; iterations {got.iterations} / {want.iterations}")
    assert differ >= 1, (name, bounds)
    assert got.state["done"] == 1.0 and abs(got.iterations - want.iterations) <= 1
    assert np.allclose(got.x, want.x, rtol=1e-6, atol=1e-6 * np.abs(want.x).max())


# ---- (d) ------------------------------------------------------------------------------------------------------------------
def test_names_are_the_sources():
    got = M.source_constants()
    assert {k: got.get(k) for k in P.PCG_SOURCE_NAMES} == P.PCG_SOURCE_NAMES
    src = {}
    for f in ("fs_cg.hip", "fs_common.h", "fs_dist.hip"):
        with open(os.path.join(M.CSRC, f)) as fh:
            src[f] = " ".join(fh.read().split())
    for name in DP.LAUNCHERS:
        assert re.search(r"\bint " + name + r"\(", src["fs_cg.hip"]), name           # defined once, beside cg_dev_*
        assert re.search(r"\bint " + name + r"\(", src["fs_common.h"]), name
        assert len(re.findall(r"\bint " + name + r"\(", src["fs_cg.hip"])) == 1, name
    for name in DP.LAUNCHERS:
        assert "fs::" + name + "(" in src["fs_dist.hip"], name                       # the sharded solvers call the same launchers
    # one copy of each step: every vector kernel is launched from ONE launcher, for whole vectors and slices alike
    for kernel in ("cg_init_kernel,", "pcg_init_kernel<true>", "pcg_start_kernel<true>", "pcg_dinv_kernel,", "cg_update_dev_kernel,",
                   "pcg_update_kernel,", "cg_direction_dev_kernel,", "pcg_direction_kernel,"):
        assert src["fs_cg.hip"].count("hipLaunchKernelGGL(" + kernel) == 1, kernel
    for kernel in ("pcgn_init_kernel", "pcgn_start_kernel", "pcgn_update_kernel", "pcgn_update_lds_kernel", "pcgn_direction_kernel"):
        # (an instantiation is named nowhere but in its launch: directly, or as one of the two forms pcgn_form_launch picks from)
        assert len(re.findall(r"(?:hipLaunchKernelGGL\(\(?|pcgn_form_launch\(k, (?:\w+<[^>]*>, )?)" + kernel + "<", src["fs_cg.hip"])) == 1, kernel
        assert len(re.findall(r"\b" + kernel + "<", src["fs_cg.hip"])) == 1, kernel
    # one dispatch from (step, sums) to the scalar step, for the whole-vector path and cg_dev_final: it knows fs_pcg's steps, each once
    for step, nvs in (("kStepPcgStart", "2"), ("kStepPcgRz", "1"), ("kStepPcgBeta", "12")):
        assert step in DP.FINAL_STEPS
        for nv in nvs:
            inst = f"final_step_kernel<{nv}, {step}>"
            assert re.search(r"case " + step + r" \* 4 \+ " + nv + r": hipLaunchKernelGGL\(\(" + inst, src["fs_cg.hip"]), inst
            assert src["fs_cg.hip"].count(inst) == 1, inst
    assert len(DP.FINAL_STEPS) == 3 and src["fs_cg.hip"].count("launch_final_step(") == 3             # defined, and its two users
    assert f"constexpr int kCgSendDoubles = {DP.SEND_DOUBLES};" in src["fs_dist.hip"]
    # the gathered rank values have block_sum<NV>'s layout: finish_sum reads part[b * NV + j], the exchange leaves rank b's NV sums
    # at b * NV
    assert "v[j] += part[b * NV + j];" in src["fs_cg.hip"] and "part[blockIdx.x * NV + threadIdx.x] = s;" in src["fs_cg.hip"]
    assert "recv[(size_t)d] + (int64_t)r * (int64_t)count" in src["fs_dist.hip"]
