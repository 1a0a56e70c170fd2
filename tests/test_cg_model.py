"""The CPU model of the CG solvers' device arithmetic (tests/_cg_model.py), pinned on the CPU:

  - its constants are the ones fs_cg.hip and fs_common.h declare, and the reduction it restates is the one the source spells out,
    so a change of launch shape fails here first rather than as an unexplained bit mismatch on the GPU;
  - with tree="serial" it is the oracle's solver (oracle/fs_oracle_cg.c) bit for bit, x and the iteration count, one and two
    right-hand sides, on every system -- so its formulas and control flow are the pinned ones and the reduction tree is the only
    difference between the model and the oracle;
  - its vectorised reduction tree is a literal per-block / per-thread / per-lane transcription of block_sum and final_sum_kernel."""
import os

import numpy as np
import pytest

import _cg_model as M
from oracle import pyoracle as O

SYSTEMS = M.systems()
PATTERN = [(n, two) for n, s in SYSTEMS.items() if s.vals is None for two in ((False, True) if s.two else (False,))]


def test_constants_are_the_sources():
    got = M.source_constants()
    want = dict(M.SOURCE_NAMES, kCgStateDone=0, kCgStateIter=1)
    assert {k: got.get(k) for k in want} == want
    assert M.CG_PART_DOUBLES >= 3 * M.RED_BLOCKS          # three partials per block (cg2) fit the part buffer
    assert max(v if isinstance(v, int) else v[0] + v[1] - 1 for v in M.ST2.values()) < M.CG_STATE_DOUBLES


def test_reduction_shape_is_the_sources():
    """the lines of fs_cg.hip the model's reduction restates"""
    with open(os.path.join(M.CSRC, "fs_cg.hip")) as f:
        src = " ".join(f.read().split())
    for line in ("for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);",
                 "if ((threadIdx.x & 63) == 0) sm[j][threadIdx.x >> 6] = s;",
                 "double s = 0.0; for (int w = 0; w < kRedThreads / 64; ++w) s += sm[threadIdx.x][w];",
                 "v[j] = 0.0; for (int b = threadIdx.x; b < nblocks; b += kRedThreads) v[j] += part[b * NV + j];",
                 "st[kStRsq] = red[0]; st[kStStop] = arg * sqrt(red[0]);",
                 "if (sqrt(rsq_new) <= st[kStStop]) st[kStDone] = 1.0;",
                 "if (n0 <= tolsq && n1 <= tolsq) st[kStDone] = 1.0;"):
        assert line in src, line
    # every grid-stride loop strides by the whole grid, and every grid is kRedBlocks x kRedThreads
    assert src.count("i += gridDim.x * kRedThreads") >= 12
    assert src.count("dim3(kRedBlocks)") + src.count("g(kRedBlocks)") >= 8
    assert "dim3(kRedBlocks), dim3(kRedThreads)" in src and "__shfl_xor(s, m)" in src


@pytest.mark.parametrize("name,two", PATTERN, ids=[f"{n}-{'cg2' if t else 'cg'}" for n, t in PATTERN])
def test_serial_model_is_the_oracle(name, two):
    s = SYSTEMS[name]
    xo, ito = O.cg_normal(s.nrow, s.ncol, s.rows, s.cols, s.B if two else s.b, s.lam, s.tol, two)
    r = s.model(two, tree="serial")
    bad = M.mismatch(r.x, xo, r.iterations, ito)
    assert bad is None, (name, two, bad)


@pytest.mark.ref
@pytest.mark.parametrize("name", ["fixture_100x50", "binary_F65", "three_eigenvalues", "cg2_zero_column"])
def test_serial_model_is_the_reference(name):
    import _cases
    import _refbind
    if not _refbind.available():
        pytest.skip("oracle/_ref not built")
    s = SYSTEMS[name]
    for two in (False, True):
        xr, itr = _cases.RefBackend().cg(s.nrow, s.ncol, s.rows, s.cols, s.B if two else s.b, s.lam, s.tol, two)
        r = s.model(two, tree="serial")
        bad = M.mismatch(r.x, xr, r.iterations, itr)
        assert bad is None, (name, two, bad)


def test_device_tree_differs_from_serial():
    """the two trees are different sums: the bit-for-bit GPU tests can tell them apart"""
    s = SYSTEMS["fixture_100x50"]
    assert not np.array_equal(s.model(tree="serial").x, s.model(tree="device").x)


# ---- the vectorised tree against a literal transcription --------------------------------------------------------------
def _literal_block(thread):
    """block_sum: the __shfl_xor butterfly of every wave, lane by lane, then lane 0 of each wave added in wave order"""
    sm = []
    for w in range(M.RED_THREADS // M.WAVE):
        s = thread[w * M.WAVE:(w + 1) * M.WAVE]
        m = M.WAVE // 2
        while m > 0:
            s = [s[lane] + s[lane ^ m] for lane in range(M.WAVE)]
            m >>= 1
        sm.append(s[0])
    total = 0.0
    for v in sm:
        total += v
    return total


def _literal_stage1(terms):
    t = [float(v) for v in terms]
    grid = M.RED_BLOCKS * M.RED_THREADS
    part = []
    for b in range(M.RED_BLOCKS):
        thread = []
        for th in range(M.RED_THREADS):
            v = 0.0
            for i in range(b * M.RED_THREADS + th, len(t), grid):
                v += t[i]
            thread.append(v)
        part.append(_literal_block(thread))
    return part


def _literal_stage2(part):
    thread = []
    for th in range(M.RED_THREADS):
        v = 0.0
        for b in range(th, len(part), M.RED_THREADS):
            v += float(part[b])
        thread.append(v)
    return _literal_block(thread)


def _hard_terms(n, seed):
    """random magnitudes over a wide range, -0.0, subnormals, and terms that cancel inside one thread, one wave, one block"""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-60, 60, n))
    if n == 0:
        return t
    k = rng.uniform(size=n)
    t[k < 0.08] = -0.0
    sub = (k >= 0.08) & (k < 0.16)
    t[sub] = rng.integers(-1000, 1000, int(sub.sum())) * 5e-324
    grid = M.RED_BLOCKS * M.RED_THREADS
    for a, d in ((0, grid), (3, 1), (5, 32), (7, 64), (11, 256)):   # x and -x meeting in a thread, a wave's tree, a block's waves
        if a + d < n:
            t[a + d] = -t[a]
    t[n // 2] = 1e300
    t[n - 1] = -1e300 if n > 1 else t[n - 1]
    return t


SIZES = [0, 1, 63, 64, 65, 256, 1000, 262_143, 262_144, 262_145, 600_000]


@pytest.mark.parametrize("n", SIZES)
def test_vectorised_tree_is_the_literal_one(n):
    t = _hard_terms(n, seed=n)
    part = M.stage1(t)
    want = _literal_stage1(t)
    assert M.same_bits(part, want).all(), (n, np.flatnonzero(~M.same_bits(part, want))[:5])
    assert M.same_bits(M.stage2(part), _literal_stage2(want)).all(), n
    if n in (0, 1000, 600_000):                                     # the three sums of cg2 are three independent trees
        t2 = _hard_terms(n, seed=n + 1)
        for terms in (t, t2):
            assert M.same_bits(M.Reducer()(terms), _literal_stage2(_literal_stage1(terms))).all()


def test_rank_combine_is_the_literal_one():
    """fs_dist_cg scheme "gather": each rank's stage 1 + 2 over its slice, then stage 2 with nblocks = number of ranks"""
    t = _hard_terms(5000, seed=3)
    bounds = [0, 1700, 1700, 5000]                                  # one rank without unknowns
    ranks = [_literal_stage2(_literal_stage1(t[lo:hi])) for lo, hi in zip(bounds[:-1], bounds[1:])]
    assert M.same_bits(M.Reducer(bounds=bounds)(t), _literal_stage2(ranks)).all()
    for nb in (1, 3, 255, 256, 257, 1024):
        p = _hard_terms(nb, seed=nb)
        assert M.same_bits(M.stage2(p), _literal_stage2(list(p))).all(), nb


def test_exact_systems_are_exact_in_the_model():
    """the exact systems of the GPU tests: x = b / 2^e (b / lam without rows) at iteration 0, with either tree"""
    for s, scale in ((M.exact_system(), 4.0), (M.exact_system(m=7, lam=9.0, F=500), 16.0), (M.exact_system(lam=0.5, nrow=0), 0.5)):
        for tree in ("device", "serial"):
            r = s.model(tree=tree)
            assert r.iterations == 0 and r.state["done"] == 1.0 and r.state["alpha"] == 1.0 / scale, (s.name, tree, r.state)
            assert M.same_bits(r.x, s.b / scale).all(), (s.name, tree)
