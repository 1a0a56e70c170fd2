"""The CPU model of fs_mscgn (tests/_mscgn_model.py), pinned on the CPU against the models it is made of:

1  its constants, the prototype and the wrapper are the sources';
2  with one column it IS the model of fs_mscg (tests/_mscg_model.py): X, the infos, the state and the per-shift scalars;
3  with one lambda it IS the model of fs_pcgn without a preconditioner from a cold start (tests/_pcgn_model.py), bit for bit, infos
   included, also under a cap of 5;
4  small ladders converge to the dense solutions of (A'A + lambda I) x = b_j: every pair converged, true residual <= 2 tol ||b_j||
   (fs_pcg's bar, as test_mscg_model.py test 4);
5  a zero column is +0.0 with 0 iterations, all its pairs converged; a NaN in one column leaves every other column's bits alone, and
   that column's pairs freeze unconverged."""
import os

import numpy as np
import pytest

import _cg_model as M
import _mscg_model as S
import _mscgn_model as SN
import _pcg_model as P
import _pcgn_model as N

SYSTEMS = M.systems(large=False)
SMALL = ("fixture_100x50", "binary_F1", "binary_F65", "three_eigenvalues", "zero_rhs", "lambda0_empty_column")
LADDER3 = (3.0, 1.0, 1.0)


def panel(s, k):
    """B (F, k): column 0 the system's b, the others deterministic and distinct"""
    i = np.arange(s.ncol, dtype=np.float64)
    return np.stack([s.b * (1.0 + 0.25 * j) + np.sin(i * (0.11 * j) + 0.3 * j) * (0.125 * j) for j in range(k)], 1)


def lams_of(s, factors):
    return [s.lam * f if s.lam else (f - 1.0) * 0.125 for f in factors]


def _products(s):
    return M.csr_products(s.nrow, s.ncol, s.a_csr(), s.t_csr_coo())[:2]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    got = M.source_constants()
    assert {k: got.get(k) for k in SN.MSCGN_SOURCE_NAMES} == SN.MSCGN_SOURCE_NAMES
    src = ""
    for f in ("fs_common.h", "fs_cg.hip"):
        with open(os.path.join(M.CSRC, f)) as fh:
            src += " ".join(fh.read().split()) + " "
    for line in SN.MSCGN_SOURCE_LINES:
        assert line in src, line
    assert 2 + 3 * SN.MAX_SHIFTS <= SN.MSCGN_SOURCE_NAMES["kSlDoubles"]
    assert SN.MAX_RHS == N.MAX_RHS and SN.MAX_SHIFTS == S.MAX_SHIFTS and got["kMscgGroup"] * SN.MAX_RHS <= M.RED_THREADS
    with open(os.path.join(M.ROOT, "include", "fastsparse_hip.h")) as f:
        hdr = " ".join(f.read().split())
    proto = ("int fs_mscgn(fs_matrix_t A, fs_matrix_t At, double *X, int64_t ldx, const double *B, int k, int m, "
             "const double *lambda /* m doubles on the HOST */, double tol, int max_iter, "
             "fs_pcg_info *info /* m * k entries, info[i * k + j], or NULL */, fs_stream_t stream);")
    assert proto in hdr
    assert hdr.index("int fs_pcgn_lambdas(") < hdr.index(proto) < hdr.index("fs_cbcsr_create(")       # behind fs_pcgn_lambdas
    assert "fs_dist_pcgn, fs_dist_pcgn_lambdas and fs_mscgn do not read it." in hdr                   # option "pcgn_compact"
    with open(os.path.join(M.ROOT, "libfastsparse_amd", "capi.py")) as f:
        capi = " ".join(f.read().split())
    assert '"fs_mscgn"' in capi and "L.fs_mscgn.argtypes = [" in capi
    assert "def mscgn(A, At, X, B, lams, tol, max_iter=0, stream=None):" in capi


def test_the_steps_are_fs_mscgs_and_the_sums_fs_pcgns():
    """one copy of the scalar lines and of the kernels that take sums: fs_mscgn calls them, it does not restate them"""
    with open(os.path.join(M.CSRC, "fs_cg.hip")) as f:
        src = " ".join(f.read().split())
    for line in ("double u = alpha * bprev; u = u * (zp - z);", "if (!(rn > stop) || fabs(zn) < 0x1p-500 || done) {",
                 "e[kMsRn] = sqrt(bb); e[kMsLive] = done ? 0.0 : 1.0;", "void mscgn_step_kernel("):
        assert src.count(line) == 1, line
    for call in ("mscg_start_step(rj[0], tol, stj, msj, m, sg, lane, active);", "mscg_s1_step(rj, stj, msj, m, lane, active);",
                 "mscg_s2_step(rj, stj, msj, m, lane, active);", "pcgn_init_step(F, k, pcgn_vec(k, X, B), false, 0.0, B, X, R, Q, U, K.tol, s)",
                 "pcgn_shift_dot_step(F, k, vec, K.sh->base, Q, P, U, s)", "pcgn_update_step(F, k, vec, nullptr, R, P, Q, nullptr, U, s)"):
        assert call in src, call
    # the pair updates: one multiply and one add for x, two multiplies and one add for a direction
    assert "const Pair x = {xv[u].a + co[u][c] * pv[u].a, V ? xv[u].b + co[u][V ? c + 1 : c] * pv[u].b : 0.0};" in src
    assert "const double t1 = zc[u][c] * r.a, t2 = bc[u][c] * pv[u].a;" in src
    assert "const Pair p = {r.a + be[c] * p0.a, V ? r.b + be[c1] * p0.b : 0.0};" in src


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_one_column_is_the_mscg_model(name):
    s = SYSTEMS[name]
    am, atm = _products(s)
    lams = lams_of(s, LADDER3)
    for cap in (0, 5):
        want = S.mscg(s.ncol, am, atm, s.b, lams, s.tol, cap)
        got = SN.mscgn(s.ncol, am, atm, s.b.reshape(-1, 1), lams, s.tol, cap)
        assert got.X.shape == (3, s.ncol, 1) and len(got.infos) == 3 and all(len(r) == 1 for r in got.infos)
        col = got.columns[0]
        bad = M.mismatch(got.X[:, :, 0], want.X, [r[0].iterations for r in got.infos], [i.iterations for i in want.infos], col.state,
                         want.state)
        assert bad is None, (name, cap, bad)
        assert S.shifts_mismatch(col.shifts, want.shifts) is None
        assert [tuple(r[0]) == tuple(w) or (np.isnan(r[0].rnorm) and np.isnan(w.rnorm)) for r, w in zip(got.infos, want.infos)] == [True] * 3


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_one_lambda_is_the_pcgn_model_without_preconditioner(name):
    s = SYSTEMS[name]
    am, atm = _products(s)
    B = panel(s, 3)
    for cap in (0, 5):
        want = N.pcgn(s.ncol, am, atm, B, s.lam, s.tol, cap)
        got = SN.mscgn(s.ncol, am, atm, B, [s.lam], s.tol, cap)
        for j in range(3):
            g, w = got.infos[0][j], want.infos[j]
            bad = M.mismatch(got.X[0][:, j], want.X[:, j], g.iterations, w.iterations, got.columns[j].state, want.columns[j].state)
            assert bad is None, (name, cap, j, bad)
            assert g.converged == w.converged and M.same_bits(g.rnorm, w.rnorm)[0] and M.same_bits(g.bnorm, w.bnorm)[0], (name, cap, j, g, w)
            assert got.columns[j].shifts["z"][0] == 1.0 and got.columns[j].shifts["pslot"][0] == -1.0


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("control", "powerlaw"))
def test_small_ladders_converge_to_the_dense_solutions(kind):
    s = P.recipe(kind, 0)
    am, atm = _products(s)
    A = P.dense(s)
    K = A.T @ A
    B = panel(s, 3)
    lams = [s.lam * f for f in (10.0, 1.0, 1e3, 1.0)]
    got = SN.mscgn(s.ncol, am, atm, B, lams, s.tol)
    for i, lam in enumerate(lams):
        Xd = np.linalg.solve(K + lam * np.eye(s.ncol), B)
        for j in range(3):
            info, x, nb = got.infos[i][j], got.X[i][:, j], np.linalg.norm(B[:, j])
            res = np.linalg.norm(K @ x + lam * x - B[:, j]) / nb
            what = (kind, i, j, info, res)
            assert info.converged == 1 and res <= 2 * s.tol and info.rnorm <= s.tol * info.bnorm, what
            # ||x - x*|| <= ||K_lam^-1|| ||residual|| <= res ||b|| / lam
            assert np.linalg.norm(x - Xd[:, j]) <= res * nb / lam * 1.01 + 1e-15 * np.linalg.norm(Xd[:, j]), what
    counts = [[got.infos[i][j].iterations for j in range(3)] for i in range(4)]
    assert counts[1] == counts[3] and all(counts[2][j] <= counts[0][j] <= counts[1][j] for j in range(3)), counts


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_a_zero_column_and_a_nan_column():
    s = SYSTEMS["binary_F65"]
    am, atm = _products(s)
    lams = lams_of(s, LADDER3)
    B = panel(s, 4)
    B[:, 2] = 0.0
    clean = SN.mscgn(s.ncol, am, atm, B, lams, s.tol, 5)
    assert all(clean.infos[i][2].iterations == 0 and clean.infos[i][2].converged == 1 for i in range(3))
    assert M.same_bits(clean.X[:, :, 2], np.zeros((3, s.ncol))).all() and not np.signbit(clean.X[:, :, 2]).any()
    Bn = B.copy()
    Bn[7, 3] = np.nan
    got = SN.mscgn(s.ncol, am, atm, Bn, lams, s.tol, 5)
    for j in (0, 1, 2):
        assert M.same_bits(got.X[:, :, j], clean.X[:, :, j]).all()
        assert [tuple(got.infos[i][j]) for i in range(3)] == [tuple(clean.infos[i][j]) for i in range(3)]
    # fs_mscg's freeze rule: !(rn > stop) holds for a NaN, so the pairs freeze unconverged; no live pair left ends the column
    assert all(got.infos[i][3].converged == 0 for i in range(3)) and got.columns[3].state["done"] == 1.0
    assert all(got.columns[3].shifts["live"] == 0.0)
