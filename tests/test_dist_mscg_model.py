"""The CPU model of fs_dist_mscg (tests/_dist_mscg_model.py), pinned on the CPU:

a  with bounds = None it IS the model of fs_mscg (tests/_mscg_model.py), bit for bit: X, the infos, the state and the per-shift
   array -- for the control / powerlaw recipes, seeds 0..2, the ladders m1 / m3 / m8, uncapped and under a cap of 5;
b  bounds whose only non-empty slice is the whole vector give the same bits (an empty slice contributes +0.0, and stage 2 over the
   rank values of one non-empty slice returns that value);
c  with the two DIFFERING_BOUNDS at least one entry of every shift's x differs from the whole tree's on the m8 ladder, the per-shift
   counts move by at most 2 and every shift converges -- so a GPU test on those cuts can tell the schemes apart;
d  m = 1 with bounds is the model of fs_dist_pcg without a preconditioner from a cold start (tests/_dist_pcg_model.py);
e  the header declares fs_dist_mscg, fs_common.h declares the launchers, fs_cg.hip defines each once and fs_dist.hip calls them; the
   Python binding exists."""
import os
import re

import numpy as np
import pytest

import _cg_model as M
import _dist_mscg_model as DS
import _dist_pcg_model as DP
import _mscg_model as S
import _pcg_model as P

SEEDS = (0, 1, 2)
KINDS = ("control", "powerlaw")
LADDERS = {"m1": (1.0,), "m3": (3.0, 1.0, 1.0), "m8": S.LADDER}
_WHOLE = {}


def _lams(s, ladder):
    return [s.lam * f for f in LADDERS[ladder]]


def _whole(kind, seed, ladder, cap):
    """the model of fs_mscg, once per case"""
    key = (kind, seed, ladder, cap)
    if key not in _WHOLE:
        s = P.recipe(kind, seed)
        _WHOLE[key] = S.run(s, _lams(s, ladder), max_iter=cap)
    return _WHOLE[key]


def _same(got, want):
    """None when X, the infos, the state and the per-shift array agree bit for bit; else what differs first"""
    bad = M.mismatch(got.X, want.X, [i.iterations for i in got.infos], [i.iterations for i in want.infos], got.state, want.state)
    if bad is None and set(got.state) != set(want.state):
        bad = f"state keys {sorted(got.state)} vs {sorted(want.state)}"
    if bad is None:
        bad = S.shifts_mismatch(got.shifts, want.shifts)
    for i, (g, w) in enumerate(zip(got.infos, want.infos)):
        if bad is None and not (g.converged == w.converged and M.same_bits(g.rnorm, w.rnorm)[0] and M.same_bits(g.bnorm, w.bnorm)[0]):
            bad = f"info[{i}]: got {g} want {w}"
    return bad


# ---- a, b ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_without_bounds_it_is_the_mscg_model(kind, seed):
    s = P.recipe(kind, seed)
    for ladder in LADDERS:
        for cap in (0, 5):
            got = DS.run(s, _lams(s, ladder), max_iter=cap)
            bad = _same(got, _whole(kind, seed, ladder, cap))
            assert bad is None, (s.name, ladder, cap, bad)


@pytest.mark.parametrize("kind", KINDS)
def test_one_slice_that_is_the_whole_vector(kind):
    s = P.recipe(kind, 0)
    F = s.ncol
    for bounds in ([0, F], [0, 0, F, F, F], [0, F, F], [0, 0, 0, F]):
        for ladder, cap in (("m8", 0), ("m3", 5)):
            got = DS.run(s, _lams(s, ladder), max_iter=cap, bounds=bounds)
            bad = _same(got, _whole(kind, 0, ladder, cap))
            assert bad is None, (s.name, bounds, ladder, cap, bad)


# ---- c ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DS.DIFFERING_BOUNDS))
def test_differing_bounds_tell_the_schemes_apart(name):
    kind = name.split("_")[0]
    s = P.recipe(kind, 0)
    assert s.name == name and s.ncol == 300
    bounds = DS.DIFFERING_BOUNDS[name]
    assert bounds == DP.DIFFERING_BOUNDS[name] and all(a < b for a, b in zip(bounds, bounds[1:])) and bounds[-1] == s.ncol
    whole = _whole(kind, 0, "m8", 0)
    sliced = DS.run(s, _lams(s, "m8"), bounds=bounds)
    differ = [int((~M.same_bits(sliced.X[i], whole.X[i])).sum()) for i in range(len(S.LADDER))]
    counts = [(w.iterations, g.iterations) for w, g in zip(whole.infos, sliced.infos)]
    print(f"{name} bounds {bounds}: entries of 300 whose bits differ per shift {differ}; counts whole / slices {counts}")
    assert min(differ) >= 1, (name, differ)
    assert all(abs(a - b) <= 2 for a, b in counts), (name, counts)
    assert all(i.converged == 1 for i in whole.infos) and all(i.converged == 1 for i in sliced.infos), name


# ---- d ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DS.DIFFERING_BOUNDS))
def test_one_lambda_with_bounds_is_the_dist_pcg_model(name):
    s = P.recipe(name.split("_")[0], 0)
    F = s.ncol
    for bounds, caps in ((DS.DIFFERING_BOUNDS[name], (0, 5)), ([0, 0, F - 1, F], (5,)), ([0, 2, 2, F - 3, F - 3, F], (5,))):
        for cap in caps:
            want = DP.run(s, P.PRECOND_NONE, max_iter=cap, bounds=bounds)
            got = DS.run(s, [s.lam], max_iter=cap, bounds=bounds)
            bad = M.mismatch(got.X[0], want.x, got.infos[0].iterations, want.iterations, got.state, want.state)
            assert bad is None, (name, bounds, cap, bad)
            assert all(k in got.state for k in want.state)
            info = got.infos[0]
            assert info.converged == int(want.state["done"]) and M.same_bits(info.rnorm, np.sqrt(want.state["rr"]))[0]
            assert M.same_bits(info.bnorm, np.sqrt(want.state["bb"]))[0]


# ---- e ---------------------------------------------------------------------------------------------------------------------
def _squeezed(*path):
    with open(os.path.join(*path)) as f:
        return " ".join(f.read().split())


SHARED_INTS = ("mscg_args_ok",)                                      # of _dist_mscg_model.SHARED, those that return a status


def test_names_are_the_sources():
    hdr = _squeezed(M.ROOT, "include", "fastsparse_hip.h")
    assert DS.PROTOTYPE in hdr
    src = {f: _squeezed(M.CSRC, f) for f in ("fs_cg.hip", "fs_common.h", "fs_dist.hip")}
    for name in DS.LAUNCHERS + SHARED_INTS:
        assert re.search(r"\bint " + name + r"\(", src["fs_common.h"]), name
        assert len(re.findall(r"\bint " + name + r"\(", src["fs_cg.hip"])) == 1, name             # defined once, beside cg_dev_*
    for name in DS.SHARED:
        assert re.search(r"\b" + name + r"\(", src["fs_common.h"]), name
        assert "fs::" + name + "(" in src["fs_dist.hip"], name
    for name in DS.LAUNCHERS:
        assert "fs::" + name + "(" in src["fs_dist.hip"], name                                    # the sharded solver calls the same launchers
    # fs_mscg itself runs on them: every mscg kernel has ONE launch site, and the host's choice of base / sigma / nslots one copy
    for kernel in ("mscg_init_kernel,", "mscg_start_kernel,", "mscg_s1_kernel,", "mscg_s2_kernel,", "mscg_update_kernel,", "mscg_direction_kernel,"):
        assert src["fs_cg.hip"].count("hipLaunchKernelGGL(" + kernel) == 1, kernel
    assert src["fs_cg.hip"].count("sg.v[i] = i < m ? lambda[i] - base : 0.0;") == 1
    assert 'mscg_args_ok("fs_mscg"' in src["fs_cg.hip"] and 'mscg_args_ok("fs_dist_mscg"' in src["fs_dist.hip"]
    assert "int fs_dist_mscg(fs_dist_matrix_t M, double *X, int64_t ldx, const double *b, int m, const double *lambda, double tol, int max_iter," in src["fs_dist.hip"]
    # the solver's work space is on the handle (one struct for both ladder solvers, an instance each) and destroy frees it
    assert src["fs_dist.hip"].count("struct LadderWork {") == 1 and "LadderWork ms, mn;" in src["fs_dist.hip"]
    assert "ensure_ladder_work(M, M->ms, m, sh.nslots," in src["fs_dist.hip"]
    destroy = src["fs_dist.hip"].split("void fs_dist_matrix_destroy(fs_dist_matrix_t M)")[1].split("delete M;")[0]
    assert "free_work(M->D, M->ms);" in destroy
    capi = _squeezed(M.ROOT, "libfastsparse_amd", "capi.py")
    assert '"fs_dist_mscg"' in capi and "def dist_mscg(M, X, b, lams, tol, max_iter=0):" in capi and "L.fs_dist_mscg.argtypes" in capi

