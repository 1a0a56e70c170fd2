"""Every CG entry point against the CPU model of its device arithmetic (tests/_cg_model.py).

(a) Under strict_order every product returns the oracle's storage-order bits, so a solve's x, its iteration count and its final
    scalars (st[], read back by fs_debug_last_cg_state) are a deterministic function the model restates: they must agree bit for
    bit -- fs_cg / fs_cg2 on handles, bsbm_cg / bsbm_cg2 through the drop-in on host structs, fs_dist_cg in both schemes and
    fs_dist_cg2 on one and three virtual ranks.
(b) On systems whose every dot is exact in any order (A'A = m I, m + lam = 2^e, dyadic b) the answer is exact in every mode:
    x = b / 2^e at iteration 0, and the iteration enqueued after convergence leaves it so.
(c) In the default modes, the bars: the residual, the distance to the model's x, the iteration count; fixed-order solves repeat
    their bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _cg_model as M
import _dist_solvers as DV
import _gpu as G
import _solvers as SV
from _gpu import FS_ERR_ARG, L  # noqa: F401

pytestmark = pytest.mark.gpu


def _cases(names=None, valued=True):
    out = []
    for n, s in SV.SYSTEMS.items():
        if (names is None or n in names) and (valued or s.vals is None):
            out += [(n, False)] + ([(n, True)] if s.two else [])
    return out


def _ids(cases):
    return [f"{n}-{'cg2' if t else 'cg'}" for n, t in cases]


# ---- (a) strict_order: bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,two", _cases(), ids=_ids(_cases()))
def test_fs_cg_strict_is_the_model(L, name, two):
    s = SV.SYSTEMS[name]
    with G.options(strict_order=1):
        x, it, st = SV.fs_cg_run(L, s, two)
    SV.assert_cg_model("fs_cg2" if two else "fs_cg", s, two, x, it, st, SV.cg_model(s, two))


@pytest.mark.parametrize("name,two", _cases(valued=False), ids=_ids(_cases(valued=False)))
def test_dropin_bsbm_cg_strict_is_the_model(L, name, two):
    s = SV.SYSTEMS[name]
    with G.options(strict_order=1):
        x, it, st, (a_csr, t_csr) = SV.dropin_run(L, s, two)
    am, atm, am2, atm2 = M.csr_products(s.nrow, s.ncol, a_csr, t_csr)
    model = M.cg2(s.ncol, am2, atm2, s.B, s.lam, s.tol) if two else M.cg(s.ncol, am, atm, s.b, s.lam, s.tol)
    SV.assert_cg_model("bsbm_cg2" if two else "bsbm_cg", s, two, x, it, st, model)


@pytest.mark.parametrize("device_t", [False, True], ids=["host-transpose", "device-transpose"])
@pytest.mark.parametrize("ranks", [1, 3])
def test_fs_dist_cg_replicate_strict_is_the_model_and_fs_cg(L, ranks, device_t):
    """scheme 0 ("replicate"): identical kernels on identical vectors -- the model's bits and fs_cg's on the same CSRs"""
    for name in SV.DIST_SET:
        s = SV.SYSTEMS[name]
        dist = DV.Dist(L, s, ranks, device_t)
        try:
            t_csr = dist.t_csr()
            want_t = s.t_csr_sorted()
            assert all(np.array_equal(a, b) for a, b in zip(t_csr[:2], want_t[:2])), (name, "A' rows are not in ascending A-row order")
            with G.options(strict_order=1, dist_cg_scheme=0):
                for two in ((False, True) if s.two else (False,)):
                    x, it, st = dist.cg(two)
                    model = SV.cg_model(s, two, "sorted")
                    entry = f"fs_dist_cg{'2' if two else ''} scheme 0, {ranks} ranks, {'device' if device_t else 'host'} A'"
                    SV.assert_cg_model(entry, s, two, x, it, st, model)
                    if not two and not device_t:
                        xs, its, sts = SV.fs_cg_run(L, s, False, t_sorted=True)
                        bad = M.mismatch(x, xs, it, its, st, sts)
                        assert bad is None, f"fs_dist_cg scheme 0 vs fs_cg on {name}: {bad}"
        finally:
            dist.close()


def test_fs_dist_cg_gather_strict_is_the_slice_model(L):
    """scheme 1 ("gather") on 3 ranks: every rank reduces its slice (the row cuts of A'), the rank values are added by stage 2"""
    for name in SV.DIST_SET:
        s = SV.SYSTEMS[name]
        for device_t in (False, True):
            dist = DV.Dist(L, s, 3, device_t)
            try:
                bounds = dist.bounds_t()
                assert bounds[0] == 0 and bounds[-1] == s.ncol
                with G.options(strict_order=1, dist_cg_scheme=1):
                    x, it, st = dist.cg(False)
                SV.assert_cg_model(f"fs_dist_cg scheme 1, 3 ranks, bounds {bounds}", s, False, x, it, st, SV.cg_model(s, False, "sorted", bounds))
            finally:
                dist.close()


# ---- (b) exact answers in every mode ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_exact_systems_single_device(L, mode):
    for s, scale in SV.EXACT:
        for two in (False, True):
            with G.mode_options(mode):
                x, it, st = SV.fs_cg_run(L, s, two)
                SV.assert_exact("fs_cg", mode, s, scale, two, x, it, st)
                x, it, st, _ = SV.dropin_run(L, s, two)
                SV.assert_exact("bsbm_cg", mode, s, scale, two, x, it, st)


@pytest.mark.parametrize("mode", G.SOLVER_MODES)
def test_exact_systems_three_ranks(L, mode):
    for s, scale in SV.EXACT[:2]:
        dist = DV.Dist(L, s, 3, False)
        try:
            for scheme in (0, 1):
                with G.mode_options(mode), G.options(dist_cg_scheme=scheme):
                    x, it, st = dist.cg(False)
                    SV.assert_exact(f"fs_dist_cg scheme {scheme}", mode, s, scale, False, x, it, st)
            with G.mode_options(mode):
                x, it, st = dist.cg(True)
                SV.assert_exact("fs_dist_cg2", mode, s, scale, True, x, it, st)
        finally:
            dist.close()


# ---- (c) default modes: the bars --------------------------------------------------------------------------------------
def _residual(s, x, two):
    """||(A'A + lam I) x - b|| / ||b|| per column, with the oracle's products"""
    am, atm, am2, atm2 = M.csr_products(s.nrow, s.ncol, s.a_csr(), s.t_csr_coo())
    if two:
        r = atm2(am2(x)) + s.lam * x - s.B
        return np.linalg.norm(r, axis=0) / np.linalg.norm(s.B, axis=0)
    return np.array([np.linalg.norm(atm(am(x)) + s.lam * x - s.b) / np.linalg.norm(s.b)])


DEFAULT_CASES = [(n, t) for n, t in _cases() if not SV.SYSTEMS[n].nan and not (t and n in ("binary_F1", "lambda0_empty_column"))]


@pytest.mark.parametrize("name,two", DEFAULT_CASES, ids=_ids(DEFAULT_CASES))
def test_default_modes_within_the_bars_of_the_model(L, name, two):
    s = SV.SYSTEMS[name]
    model = SV.cg_model(s, two)
    res_m = _residual(s, model.x, two)
    bnorm = np.linalg.norm(s.B if two else s.b, axis=0) if two else np.array([np.linalg.norm(s.b)])
    for mode in ("default", "cg_fixed_order=0"):
        with G.mode_options(mode):
            runs = [SV.fs_cg_run(L, s, two) for _ in range(2)]
        x, it, _ = runs[0]
        what = (name, two, mode, it, model.iterations)
        res = _residual(s, x, two)
        if s.converges and not (two and name == "three_eigenvalues"):   # (two columns on three unknowns: the cap ends it)
            assert np.all(res <= 2 * s.tol), (what, res)
        if s.lam > 0:                                           # ||(A'A + lam I)^-1|| <= 1 / lam: holds for any two x
            err = np.linalg.norm((x - model.x).reshape(s.ncol, -1), axis=0)
            assert np.all(err <= (res + res_m) * bnorm / s.lam * 1.01 + 1e-300), (what, err, res, res_m)
        if s.well:
            assert abs(it - model.iterations) <= 1, what
        else:
            assert it <= s.ncol, what
        if mode == "default":                                   # fixed-order products: a solve repeats its bits
            assert runs[1][1] == it and M.same_bits(runs[1][0], x).all(), what


# ---- statuses ----------------------------------------------------------------------------------------------------------------
def test_statuses(L):
    """fs_cg / fs_cg2 refuse a NULL argument and an At of A's own shape with FS_ERR_ARG and a message, before anything is written
    to x; out_iter = NULL is legal"""
    import torch
    from libfastsparse_amd import capi
    s = SV.SYSTEMS["fixture_100x50"]
    A = capi.Matrix.from_coo(s.nrow, s.ncol, G.to_device(s.rows), G.to_device(s.cols), None)
    At = capi.Matrix.from_coo(s.ncol, s.nrow, G.to_device(s.cols), G.to_device(s.rows), None)
    st = capi.current_stream()
    for f, rhs in ((L.fs_cg, s.b), (L.fs_cg2, s.B)):
        b = G.to_device(rhs.reshape(-1))
        x = torch.full((rhs.size,), float("nan"), dtype=torch.float64, device="cuda")
        x_bits = x.cpu().numpy().view(np.int64).copy()
        good = dict(A=A.h, At=At.h, x=x.data_ptr(), b=b.data_ptr())
        for what, kw in (("NULL A", dict(A=None)), ("NULL At", dict(At=None)), ("NULL x", dict(x=None)), ("NULL b", dict(b=None)),
                         ("At is A", dict(At=A.h))):
            a = dict(good, **kw)
            rc = f(a["A"], a["At"], a["x"], a["b"], s.lam, s.tol, None, st)
            assert rc == FS_ERR_ARG, (f.__name__, what, rc)
            assert L.fs_last_error().startswith(f.__name__.encode() + b":"), (f.__name__, what, L.fs_last_error())   # its own message
        SV.refused_call_leaves(x, x_bits, f"{f.__name__}: a refused call wrote to x")
        assert f(A.h, At.h, x.data_ptr(), b.data_ptr(), s.lam, s.tol, None, st) == 0, L.fs_last_error()   # out_iter NULL is legal


# ---- the drop-in on three virtual ranks -----------------------------------------------------------------------------------
def test_dropin_cg_across_three_ranks_in_a_child_process(L):
    """FASTSPARSE_NGPU=3 FASTSPARSE_DEVICES=0,0,0: bsbm_cg / bsbm_cg2 on the row-sharded path -- strict_order bits against the
    model, exact answers in every mode (tests/_dropin_ngpu.py, mode `cg`)"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dropin_ngpu.py")
    env = dict(os.environ, FASTSPARSE_NGPU="3", FASTSPARSE_DEVICES="0,0,0")
    p = subprocess.run([sys.executable, child, "cg"], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), p.stdout[-3000:] + p.stderr[-3000:]
