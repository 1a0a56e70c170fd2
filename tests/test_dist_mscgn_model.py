"""The CPU model of fs_dist_mscgn (tests/_dist_mscgn_model.py), pinned on the CPU:

a  the header declares fs_dist_mscgn, fs_common.h declares the launchers, fs_cg.hip defines each once, fs_mscgn and fs_dist.hip call
   them; the step over the gathered sums is pcgn_fold_kernel's own fold, launched from one site; the Python binding exists;
b  with bounds = None it IS the model of fs_mscgn (tests/_mscgn_model.py), bit for bit: X, the infos, every column's state and
   per-shift array -- the eight-column recipes, ladders m3 and m8, uncapped and under a cap of 5;
c  with the two DIFFERING_BOUNDS the slice model differs from the whole model in at least half of the non-zero columns, on the
   ladders m3 and m8 -- so a GPU test on those cuts can tell the schemes apart; every pair converges either way;
d  bounds whose only non-empty slice is the whole panel give the whole model's bits; the cache returns the same objects."""
import os
import re

import numpy as np
import pytest

import _cg_model as M
import _dist_mscgn_model as DN
import _mscg_model as S
import _mscgn_model as SN
import _pcgn_model as N

KINDS = ("control", "powerlaw")
LADDERS = {"m3": (3.0, 1.0, 1.0), "m8": S.LADDER}
_CACHE = {}


def _lams(s, ladder):
    return [s.lam * f for f in LADDERS[ladder]]


def _columns_mismatch(got, want):
    """None when X, the infos and every column's state and per-shift array agree bit for bit; else what differs first"""
    if got.X.shape != want.X.shape:
        return f"X shape {got.X.shape} != {want.X.shape}"
    for j, (g, w) in enumerate(zip(got.columns, want.columns)):
        bad = M.mismatch(g.X, w.X, [i.iterations for i in g.infos], [i.iterations for i in w.infos], g.state, w.state)
        if bad is None:
            bad = S.shifts_mismatch(g.shifts, w.shifts)
        if bad is None and not M.same_bits(got.X[:, :, j], w.X).all():
            bad = "the panels do not hold the column's x"
        for i, (a, b) in enumerate(zip(g.infos, w.infos)):
            if bad is None and not (a.converged == b.converged and M.same_bits(a.rnorm, b.rnorm)[0] and M.same_bits(a.bnorm, b.bnorm)[0]):
                bad = f"info[{i}]: got {a} want {b}"
        if bad is not None:
            return f"column {j}: {bad}"
    return None


# ---- a ---------------------------------------------------------------------------------------------------------------------
def _squeezed(*path):
    with open(os.path.join(*path)) as f:
        return " ".join(f.read().split())


def test_names_are_the_sources():
    hdr = _squeezed(M.ROOT, "include", "fastsparse_hip.h")
    assert DN.PROTOTYPE in hdr
    assert hdr.index("int fs_dist_mscg(") < hdr.index(DN.PROTOTYPE) < hdr.index("int fs_dist_spmm(")          # behind fs_dist_mscg
    src = {f: _squeezed(M.CSRC, f) for f in ("fs_cg.hip", "fs_common.h", "fs_dist.hip")}
    cg = src["fs_cg.hip"]
    for name in DN.LAUNCHERS:
        assert re.search(r"\bint " + name + r"\(", src["fs_common.h"]), name
        assert len(re.findall(r"\bint " + name + r"\(", cg)) == 1, name                                # defined once, beside mscg_dev_*
        assert "fs::" + name + "(" in src["fs_dist.hip"], name                                         # the sharded solver calls them
    for name in DN.SHARED:
        assert re.search(r"\b" + name + r"\(", src["fs_common.h"]), name
        assert "fs::" + name + "(" in src["fs_dist.hip"], name
    # fs_mscgn itself runs on them, and every kernel of it has ONE launch site per instantiation
    assert "mscgn_dev_init(F, k, B, X, (long long)ldx, f.r, f.p, f.q, Ps, ldp, U, K, s)" in cg
    assert "mscgn_dev_steps(F, k, X, (long long)ldx, f.r, f.p, f.q, Ps, ldp, U, K, s)" in cg
    for kernel in ("mscgn_step_kernel<kMscgStart>,", "mscgn_step_kernel<kMscgS1>,", "mscgn_step_kernel<kMscgS2>,", "mscgn_fill_kernel<true>,",
                   "mscgn_update_kernel<true>,", "mscgn_direction_kernel<true>,", "mscgn_fill_kernel<false>,", "mscgn_update_kernel<false>,",
                   "mscgn_direction_kernel<false>,", "pcgn_fold_kernel,"):
        assert cg.count("hipLaunchKernelGGL(" + kernel) == 1, kernel
    # the flat pair kernels have no slice form, the scalar lines one copy
    for once in ("void mscgn_fill_kernel(", "void mscgn_update_kernel(", "void mscgn_direction_kernel(", "void mscgn_step_kernel(",
                 "void pcgn_fold_kernel("):
        assert cg.count(once) == 1, once
    # the gathered sums: pcgn_step_kernel<STEP, true>'s fold, then the same four wave sums
    assert "if (ranks > 0) pcgn_fold<true>(part, ranks, live, nv, ns, sm);" in cg
    assert "pcgn_fold_launch(all, nranks, K.red, U.st, k, step == kMscgStart ? 2 : 1, step == kMscgStart, s);" in cg
    assert 'mscg_args_ok("fs_dist_mscgn"' in src["fs_dist.hip"]
    assert ("int fs_dist_mscgn(fs_dist_matrix_t M, double *X, int64_t ldx, const double *B, int k, int m, const double *lambda, double tol, "
            "int max_iter,") in src["fs_dist.hip"]
    # the solver's work space is on the handle (one struct for both ladder solvers, an instance each) and destroy frees both
    dist = src["fs_dist.hip"]
    assert dist.count("struct LadderWork {") == 1 and "LadderWork ms, mn;" in dist
    assert "ensure_ladder_work(M, M->mn, m, sh.nslots," in dist
    destroy = dist.split("void fs_dist_matrix_destroy(fs_dist_matrix_t M)")[1].split("delete M;")[0]
    assert "free_work(M->D, M->ms);" in destroy and "free_work(M->D, M->mn);" in destroy
    assert 'DistSolve f{"fs_dist_mscgn", M};' in dist and "ensure_pn_work(M, k, gather)" in dist
    # what the sharded solvers share exists once: the exchange of sums (its event record, its slot flip), the slice geometry (no
    # solver declares its own), and the host loop that holds every rank's outcome against rank 0's, with each solver's own text
    assert dist.count("hipEventRecord(T.ev[") == 1 and dist.count("slot ^= 1;") == 1       # (the staged uploads flip a slot of their own)
    assert "auto lo_of" not in dist and "auto rows_of" not in dist
    for what in ("columns", "shifts", "pairs"):
        assert dist.count("the devices froze the " + what + " differently (a device or an exchange returned different bits)") == 1, what
    assert dist.count("int agree(Agreement &a)") == 1 and dist.count("fs::set_error(a.differ)") == 1
    assert "if (int rc = agree(*also)) return rc;" in dist and dist.count("_same_outcome(") == 3      # finish() runs it; a comparison per solver
    capi = _squeezed(M.ROOT, "libfastsparse_amd", "capi.py")
    assert '"fs_dist_mscgn"' in capi and "def dist_mscgn(M, X, B, lams, tol, max_iter=0):" in capi and "L.fs_dist_mscgn.argtypes" in capi


# ---- b ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_without_bounds_it_is_the_mscgn_model(kind):
    s, B, _ = N.recipe8(kind)
    for ladder in LADDERS:
        for cap in (0, 5):
            want = SN.run(s, B, _lams(s, ladder), max_iter=cap)
            got = DN.run(s, B, _lams(s, ladder), max_iter=cap, cache=_CACHE)
            bad = _columns_mismatch(got, want)
            assert bad is None, (s.name, ladder, cap, bad)
            assert [[tuple(i) for i in row] for row in got.infos] == [[tuple(i) for i in row] for row in want.infos]


# ---- c ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ladder", list(LADDERS))
@pytest.mark.parametrize("name", list(DN.DIFFERING_BOUNDS))
def test_differing_bounds_tell_the_schemes_apart(name, ladder):
    kind = name.split("_")[0]
    s, B, _ = N.recipe8(kind)
    assert s.name == name and s.ncol == 300 and B.shape == (300, 8)
    bounds = DN.DIFFERING_BOUNDS[name]
    nonzero = [j for j in range(8) if B[:, j].any()]
    assert len(nonzero) == 7
    whole = DN.run(s, B, _lams(s, ladder), cache=_CACHE)
    sliced = DN.run(s, B, _lams(s, ladder), bounds=bounds, cache=_CACHE)
    differ = DN.differing_columns(sliced, whole)
    its = max(i.iterations for row in sliced.infos for i in row)
    print(f"{name} {ladder} bounds {bounds}: columns whose bits differ {differ} of the non-zero {nonzero}; longest pair {its} iterations")
    assert set(differ) <= set(nonzero) and 2 * len(differ) >= len(nonzero), (name, ladder, differ)
    for r in (whole, sliced):
        assert all(i.converged == 1 for row in r.infos for i in row), (name, ladder)


# ---- d ---------------------------------------------------------------------------------------------------------------------
def test_one_slice_that_is_the_whole_panel_and_the_cache():
    s, B, _ = N.recipe8("control")
    F = s.ncol
    lams = _lams(s, "m3")
    want = DN.run(s, B, lams, max_iter=5, cache=_CACHE)
    for bounds in ([0, F], [0, 0, F, F, F], [0, 0, 0, F]):
        got = DN.run(s, B[:, :3], lams, max_iter=5, bounds=bounds)
        bad = _columns_mismatch(got, SN._gather(want.columns[:3], 3))
        assert bad is None, (bounds, bad)
    again = DN.run(s, B, lams, max_iter=5, cache=_CACHE)
    assert all(a is b for a, b in zip(again.columns, want.columns))
    other = DN.run(s, B, lams, max_iter=5, bounds=[0, 100, 200, 300], cache=_CACHE)                # the bounds are part of the key
    assert not any(a is b for a, b in zip(other.columns, want.columns))
    sorted_t = DN.run(s, B, lams, max_iter=5, t_csr=s.t_csr_sorted(), cache=_CACHE)                # and so are the arrays of A'
    assert not any(a is b for a, b in zip(sorted_t.columns, want.columns))


@pytest.mark.parametrize("F,nrow,bounds,k,m", [(300, 2000, [0, 100, 200, 300], 5, 8), (3, 3, [0, 1, 2, 3, 3, 3], 3, 3)])
def test_the_poisoned_sizes_are_the_headers_work_space_per_rank(F, nrow, bounds, k, m):
    """_dist_solvers.work_space_per_rank -- what the dirty-work suite poisons before a sharded solve makes its work space -- holds
    every term of include/fastsparse_hip.h, "Work space per rank" (fs_dist_pcgn_lambdas, fs_dist_mscgn; fs_dist_mscg's (m + nslots) F
    divided by the ranks), with the sizes the sources give the constants: a size that is off makes the poison miss silently"""
    import _dist_solvers as DV
    text = " ".join(open(os.path.join(M.ROOT, "include", "fastsparse_hip.h")).read().split())
    for words in ("Work space per rank: five slices of n_r k * doubles (X, R, B, Q, and P in the send buffer), the whole P (ncol k) and T (nrow k), the slice of s / dinv, the partials, "
                  "* two send slots of 2 FS_PCGN_MAX_RHS doubles and N times that for the gathered values",
                  "m + nslots panels of n_r k doubles * (rounded up to an even count) for the X_i and the P_i",
                  "2048 k doubles of partial sums, two send slots of 2 FS_PCGN_MAX_RHS doubles and N times * that for the gathered values; 9344 doubles of scalars",
                  "as is the * (m + nslots) F work space"):
        assert words in text, words
    src = open(os.path.join(M.CSRC, "fs_common.h")).read() + open(os.path.join(M.CSRC, "fs_dist.hip")).read()
    for line in ("constexpr size_t pcgn_part_doubles(int k) { return (size_t)1024 * 2 * (size_t)k; }", "constexpr int kPcgnSendDoubles = 2 * FS_PCGN_MAX_RHS;",
                 "const size_t fl = (size_t)(F ? F : 1) + (size_t)M->t.plan.max_rows + 1;"):
        assert line in src, line
    n = len(bounds) - 1
    rows = [b - a for a, b in zip(bounds, bounds[1:])]
    even = lambda v: (v + 1) & ~1
    nslots, send = m - 1, 2 * N.MAX_RHS
    nl = DV.work_space_per_rank("pcgn_lambdas", F, nrow, bounds, k, scheme=1)
    assert {max(r, 1) * k for r in rows} | {F * k, nrow * k} | {max(r, 1) for r in rows} | {2048 * k, 2 * send, n * send} <= set(nl), nl
    whole = DV.work_space_per_rank("pcgn_lambdas", F, nrow, bounds, k, scheme=0)
    assert {F * k, nrow * k, F, 2048 * k} <= set(whole) and 2 * send not in whole, whole
    assert DV.work_space_per_rank("pcgn", F, nrow, bounds, k, scheme=1) == DV.work_space_per_rank("pcgn", F, nrow, bounds, k, scheme=0)
    for scheme, n_r in ((0, F), (1, max(rows))):
        mn = DV.work_space_per_rank("mscgn", F, nrow, bounds, k, m, nslots, scheme)
        assert {even(n_r * k) * m, even(n_r * k) * nslots, 9344, 2048 * k, F * k, nrow * k} <= set(mn), (scheme, mn)
        ms = DV.work_space_per_rank("mscg", F, nrow, bounds, 1, m, nslots, scheme)
        assert {even(n_r) * m, even(n_r) * nslots, S.MAX_SHIFTS * S.MS_STRIDE, F + max(rows) + 1, M.CG_PART_DOUBLES} <= set(ms), (scheme, ms)
    assert DV.MN_SCALARS == 9344 and 2 * M.RED_BLOCKS == 2048
