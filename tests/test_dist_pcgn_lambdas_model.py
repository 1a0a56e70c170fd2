"""fs_dist_pcgn_lambdas on the CPU: its interface against the sources and its model (tests/_dist_pcgn_lambdas_model.py: column j is the
model of fs_dist_pcg at that column's lambda).

1  the header declares the function, capi.py lists and wraps it; every k-column vector kernel still has ONE launch site, the slice
   steps and the rank step are launchers of fs_cg.hip declared in fs_common.h and called from fs_dist.hip; the k-wide send slots
   have a constant of their own and the rank step reads the gathered values where the exchange leaves them.
2  with bounds=None the model is _pcgn_lambdas_model.run, bit for bit (scheme 0 is fs_pcgn_lambdas).
3  on the eight-column recipes with a ladder of lambdas, Jacobi and three non-empty slices the slice model and the whole model
   differ in at least 4 of the 8 columns (which is what lets the GPU test tell scheme 1 from scheme 0); the zero column never
   does, and the iteration counts agree."""
import os
import re

import numpy as np
import pytest

import _cg_model as M
import _dist_pcg_model as DP
import _dist_pcgn_lambdas_model as DNL
import _pcg_model as P
import _pcgn_lambdas_model as NL
import _pcgn_model as N


def _squeezed(*path):
    with open(os.path.join(*path)) as f:
        return " ".join(f.read().split())


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def test_interface_is_the_sources():
    hdr = _squeezed(M.ROOT, "include", "fastsparse_hip.h")
    proto = ("int fs_dist_pcgn_lambdas(fs_dist_matrix_t M, double *X, const double *B, int k, "
             "const double *lambda /* k doubles on the HOST */, const fs_pcg_params *prm, fs_pcg_info *info /* k entries or NULL */);")
    assert proto in hdr
    assert hdr.index("int fs_dist_pcgn(") < hdr.index(proto) < hdr.index("int fs_dist_mscg(")      # behind fs_dist_pcgn
    capi = _squeezed(M.ROOT, "libfastsparse_amd", "capi.py")
    assert '"fs_dist_pcgn_lambdas"' in capi and "L.fs_dist_pcgn_lambdas.argtypes = [" in capi
    assert ("def dist_pcgn_lambdas(M, X, B, lams, tol, max_iter=0, precond=FS_PRECOND_JACOBI, warm_start=False, diag=None):") in capi


def test_launchers_are_the_sources():
    src = {f: _squeezed(M.CSRC, f) for f in ("fs_cg.hip", "fs_common.h", "fs_dist.hip")}
    cg = src["fs_cg.hip"]
    # one launch site per vector kernel, for whole panels and slices, fs_pcgn and fs_pcgn_lambdas alike
    for kernel in ("pcgn_init_kernel", "pcgn_start_kernel", "pcgn_shift_dot_kernel", "pcgn_shift_dot_lds_kernel", "pcgn_update_kernel",
                   "pcgn_update_lds_kernel", "pcgn_direction_kernel", "pcgn_direction_lds_kernel"):
        # (an instantiation is named nowhere but in its launch: directly, or as one of the two forms pcgn_form_launch picks from)
        assert len(re.findall(r"(?:hipLaunchKernelGGL\(\(?|pcgn_form_launch\(k, (?:\w+<[^>]*>, )?)" + kernel + "<", cg)) == 1, kernel
        assert len(re.findall(r"\b" + kernel + "<", cg)) == 1, kernel
    assert cg.count("hipLaunchKernelGGL(kernel, dim3(kRedBlocks), dim3(kRedThreads), 0, s, a...);") == 1
    assert cg.count("hipLaunchKernelGGL(pcgn_fold_kernel,") == 1
    # one copy of the scalar lines: the step kernel is defined once and instantiated for partials and for gathered rank values
    assert cg.count("void pcgn_step_kernel(") == 1 and cg.count("e[kPnAlpha] = e[kPnRz] / s0;") == 1
    assert "pcgn_step_kernel<kPnStepBeta, RANKS>" in cg and "pcgn_step_launch<true>(" in cg and "pcgn_step_launch<false>(" in cg
    # the gathered values: rank b's nv sums at b * nv, where the exchange leaves them
    assert "a[u] += part[(size_t)b * nv + v];" in cg
    assert "recv[(size_t)d] + (int64_t)r * (int64_t)count" in src["fs_dist.hip"]
    # a k-column exchange carries ns * k doubles per rank, on the compute streams: the count the k-column callers hand to the one
    # combine, whose exchange_equal call is the only one on D->stream
    assert "SliceSums sums{M, W.send, W.all, fs::kPcgnSendDoubles};" in src["fs_dist.hip"]
    assert "return sums.combine((size_t)ns * (size_t)k, [&](int d, const double *all) {" in src["fs_dist.hip"]
    assert src["fs_dist.hip"].count("exchange_equal(D, from, all, count, D->stream, ready)") == 1
    assert src["fs_dist.hip"].count("D->stream, ready)") == 1
    for name in ("pcgn_dev_init_lambdas", "pcgn_dev_steps_lambdas", "pcgn_slice_init", "pcgn_slice_start", "pcgn_slice_shift_dot",
                 "pcgn_slice_update", "pcgn_slice_direction", "pcgn_dev_rank_step"):
        assert len(re.findall(r"\bint " + name + r"\(", cg)) == 1, name
        assert re.search(r"\bint " + name + r"\(", src["fs_common.h"]), name
        assert "fs::" + name + "(" in src["fs_dist.hip"], name
    assert "constexpr int kPcgnSendDoubles = 2 * FS_PCGN_MAX_RHS;" in src["fs_common.h"]
    assert f"constexpr int kCgSendDoubles = {DP.SEND_DOUBLES};" in src["fs_dist.hip"]
    # the diagonal at 0.0, no inverse pass: whole (gathered once) or the rank's own rows
    assert "gram_diag_everywhere(M, 0.0, W.dinv)" in src["fs_dist.hip"] and "gram_diag_slices(M, 0.0, W.dinv)" in src["fs_dist.hip"]


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", (P.PRECOND_NONE, P.PRECOND_JACOBI, P.PRECOND_DIAG))
def test_without_bounds_it_is_the_pcgn_lambdas_model(precond):
    s = M.systems(large=False)["binary_F65"]
    k = 3
    lams = NL.rungs(s, k)
    i = np.arange(s.ncol, dtype=np.float64)
    B = np.stack([s.b * (1.0 + j) + np.sin(i * 0.3 * j) for j in range(k)], 1)
    X0 = np.stack([0.01 * np.cos(i * 0.7 + j) for j in range(k)], 1)
    diag = np.abs(P.gram_diag(s.t_csr_coo(), s.lam)) * (1.0 + 0.5 * np.cos(i * 1.7)) + 0.125 if precond == P.PRECOND_DIAG else None
    for x0s, cap in ((None, 0), (X0, 3)):
        want = NL.run(s, B, lams, precond, max_iter=cap, X0=x0s, diag=diag)
        for bounds in (None, [0, 0, s.ncol, s.ncol]):                 # (empty slices give +0.0: still the whole tree)
            got = DNL.run(s, B, lams, precond, max_iter=cap, X0=x0s, diag=diag, bounds=bounds)
            for j in range(k):
                bad = M.mismatch(got.X[:, j], want.X[:, j], got.infos[j].iterations, want.infos[j].iterations, got.columns[j].state,
                                 want.columns[j].state)
                assert bad is None, (precond, cap, bounds, j, bad)
                assert got.infos[j].converged == want.infos[j].converged


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("control", "powerlaw"))
def test_three_slices_round_differently_in_half_the_columns(kind):
    s, B, _ = N.recipe8(kind)
    lams = NL.rungs(s, 8)
    bounds = DP.DIFFERING_BOUNDS[s.name]
    assert bounds[0] == 0 and bounds[-1] == s.ncol and all(a < b for a, b in zip(bounds, bounds[1:]))
    whole = DNL.run(s, B, lams, P.PRECOND_JACOBI)
    sliced = DNL.run(s, B, lams, P.PRECOND_JACOBI, bounds=bounds)
    differ = [not M.same_bits(whole.X[:, j], sliced.X[:, j]).all() for j in range(8)]
    counts = [(a.iterations, b.iterations) for a, b in zip(whole.infos, sliced.infos)]
    print(f"{s.name} bounds {bounds}: columns that differ {differ}; iterations (whole, sliced) {counts}")
    assert sum(differ) >= 4, (s.name, differ)
    assert DNL.columns_that_differ(whole, sliced) == sum(differ)
    assert not differ[3] and sliced.infos[3].iterations == 0 and M.same_bits(sliced.X[:, 3], np.zeros(s.ncol)).all()
    assert all(i.converged == 1 for i in sliced.infos)
    assert all(a == b for a, b in counts), counts
    assert np.allclose(sliced.X, whole.X, rtol=1e-6, atol=1e-6 * np.abs(whole.X).max(0))
