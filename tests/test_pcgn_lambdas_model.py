"""fs_pcgn_lambdas on the CPU: its interface against the sources, its model (tests/_pcgn_lambdas_model.py: column j is the model of
fs_pcg at that column's lambda), the one fact about fs_gram_diag that lets a solve form every column's diagonal from one pass, and the
facts about a ladder of lambdas that the entry point rests on.

1  the header declares the function, capi.py lists and wraps it; the kernels keep fs_pcgn's lines and carry the per-column ones.
2  the model's column j is _pcg_model.pcg at lams[j] with that column's dinv, for none, Jacobi and a caller's diagonal.
3  gram_diag(t_csr, 0.0) + lam has the bits of gram_diag(t_csr, lam) for every rung on the nine recipes, and on
   lambda0_empty_column and valued with lambda = 0 among the rungs.
4  the ladder on the nine recipes: with the Jacobi diagonal of its own lambda every rung converges, true residual <= 2 tol against
   the dense system; on the column-scaled recipes plain CG ends at the cap on the seven smallest rungs and ONE shared diagonal (the
   smallest lambda's) needs more than twice the per-column count at the three largest rungs; on the scaled and power-law recipes the
   per-column counts differ over the ladder, so columns freeze at different iterations."""
import os

import numpy as np
import pytest

import _cg_model as M
import _pcg_model as P
import _pcgn_lambdas_model as NL

KINDS = ("scaled", "powerlaw", "control")
RECIPES = [(k, seed) for k in KINDS for seed in (0, 1, 2)]
_LADDER = {}


def _squeezed(*path):
    with open(os.path.join(*path)) as f:
        return " ".join(f.read().split())


def _ladder(kind, seed):
    """the recipe, its 8 rungs and the per-column Jacobi solves of b at every rung (computed once)"""
    if (kind, seed) not in _LADDER:
        s = P.recipe(kind, seed)
        lams = NL.rungs(s, 8)
        B = np.repeat(s.b[:, None], 8, 1)
        _LADDER[kind, seed] = (s, lams, NL.run(s, B, lams, P.PRECOND_JACOBI))
    return _LADDER[kind, seed]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def test_interface_is_the_sources():
    hdr = _squeezed(M.ROOT, "include", "fastsparse_hip.h")
    assert ("int fs_pcgn_lambdas(fs_matrix_t A, fs_matrix_t At, double *X, const double *B, int k, "
            "const double *lambda /* k doubles on the HOST */, const fs_pcg_params *prm, "
            "fs_pcg_info *info /* k entries or NULL */, fs_stream_t stream);") in hdr
    capi = _squeezed(M.ROOT, "libfastsparse_amd", "capi.py")
    assert '"fs_pcgn_lambdas"' in capi
    assert ("def pcgn_lambdas(A, At, X, B, lams, tol, max_iter=0, precond=FS_PRECOND_JACOBI, warm_start=False, diag=None, "
            "stream=None):") in capi
    common = _squeezed(M.CSRC, "fs_common.h")
    assert "struct PcgnLambdas { double v[FS_PCGN_MAX_RHS]; };" in common


def test_arithmetic_is_the_sources():
    """the per-column lines of fs_cg.hip that the model restates: fs_pcgn's lines with lambda.v[c] for lambda and, where the diagonal
    follows the column, pn_inv(s, lambda_c) for di; pn_inv is pcg_dinv_kernel's line on s + lambda"""
    src = _squeezed(M.CSRC, "fs_cg.hip")
    for line in ("const double d = s + lambda; return d == 0.0 ? 1.0 : 1.0 / d;",
                 "dinv[i] = di == 0.0 ? 1.0 : 1.0 / di;",
                 # column c's lambda: by value in the lane-per-row kernels, from the table in LDS in the staged ones
                 "double pn_lambda(const PcgnLambdas &lambda, int c) { return lambda.v[c]; }",
                 "double pn_lambda(const double *lam, int c) { return lam[c]; }",
                 "__shared__ double lam[KMAX]; if (threadIdx.x < KMAX) lam[threadIdx.x] = lambda.v[threadIdx.x]; return lam;",
                 # init (warm), shift-dot: fs_pcgn's lines with pn_lambda(lambda, c)
                 "const Pair r = {pn_init(warm, q.a, pn_lambda(lambda, c), x.a, b.a, bb[c], rr[c]), "
                 "pn_init(warm, q.b, pn_lambda(lambda, c + 1), x.b, b.b, bb[c + 1], rr[c + 1])};",
                 "const Pair q = {pn_shift_dot(q0.a, pn_lambda(lambda, c), p.a, qp[c]), pn_shift_dot(q0.b, pn_lambda(lambda, c + 1), p.b, qp[c + 1])};",
                 "const auto lam = pl_lambdas<KMAX>(lambda);",
                 "pass(Q, P, nullptr, [&](int c, double q0, double p, double) { return pn_shift_dot(q0, pn_lambda(lam, c), p, qp[c]); });",
                 # start, update, direction: z = r dinv_c
                 "else return r * pn_inv(di, pn_lambda(colj, c));",
                 "const auto &colj = pn_colj(lambda...);",
                 "const auto colj = pl_lambdas<KMAX>(lambda...);",
                 "const PcgnLambdas &pn_colj(const PcgnLambdas &lambda) { return lambda; }",
                 "if (sizeof...(LAM) != 0 || dinv) rz[c] += r * pn_z(r, dinv != nullptr, di, colj, c);",
                 "return pn_direction(pn_z(r, dinv != nullptr, di, colj, c), be[c], p0);",
                 # the host: one s per solve, no inverse pass
                 "if (int rc = fs_gram_diag(At, colj ? 0.0 : lambda, dinv, stream)) return rc;",
                 "if (pre && !colj)"):
        assert line in src, line
    # one copy of the per-column inverse; the three lane-per-row kernels and the two staged ones that form z take it through pn_z
    assert src.count("pn_inv(") == 2 and src.count("const auto &colj = pn_colj(lambda...);") == 3
    assert src.count("const auto colj = pl_lambdas<KMAX>(lambda...);") == 2
    assert "-ffast-math" not in _squeezed(M.ROOT, "libfastsparse_amd", "_build.py")      # 1.0 / d stays an IEEE division
    assert "-ffp-contract=off" in _squeezed(M.ROOT, "libfastsparse_amd", "_build.py")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", (P.PRECOND_NONE, P.PRECOND_JACOBI, P.PRECOND_DIAG))
def test_model_columns_are_fs_pcgs_model(precond):
    s = M.systems(large=False)["binary_F65"]
    t_csr = s.t_csr_coo()
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr)
    k = 3
    lams = NL.rungs(s, k)
    assert len(set(lams)) == k and lams[0] == s.lam
    i = np.arange(s.ncol, dtype=np.float64)
    B = np.stack([s.b * (1.0 + j) + np.sin(i * 0.3 * j) for j in range(k)], 1)
    X0 = np.stack([0.01 * np.cos(i * 0.7 + j) for j in range(k)], 1)
    diag = np.abs(P.gram_diag(t_csr, s.lam)) * (1.0 + 0.5 * np.cos(i * 1.7)) + 0.125 if precond == P.PRECOND_DIAG else None
    for x0s, cap in ((None, 0), (X0, 3)):
        got = NL.run(s, B, lams, precond, max_iter=cap, X0=x0s, diag=diag)
        dinvs = [NL.dinv_of_column(t_csr, lam, precond, diag) for lam in lams]
        also = NL.pcgn_lambdas(s.ncol, am, atm, B, lams, s.tol, cap, None if precond == P.PRECOND_NONE else dinvs, x0s)
        for j in range(k):
            dinv = {P.PRECOND_NONE: None, P.PRECOND_JACOBI: P.dinv_of(P.gram_diag(t_csr, lams[j])), P.PRECOND_DIAG: P.dinv_of(diag)}[precond]
            want = P.pcg(s.ncol, am, atm, B[:, j], lams[j], s.tol, cap, dinv, None if x0s is None else x0s[:, j])
            for res in (got, also):
                assert M.mismatch(res.X[:, j], want.x, res.infos[j].iterations, want.iterations, res.columns[j].state, want.state) is None
                assert res.infos[j].converged == int(want.state["done"])
        if precond != P.PRECOND_NONE and not cap:
            assert len({i.iterations for i in got.infos}) >= 2       # the columns are different solves


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def _assert_sum_plus_lambda(name, t_csr, lams):
    zero = P.gram_diag(t_csr, 0.0)
    assert not np.signbit(zero).any(), name                          # a sum of squares from +0.0 is never -0.0
    for lam in lams:
        got, want = zero + np.float64(lam), P.gram_diag(t_csr, lam)
        assert M.same_bits(got, want).all(), (name, lam)


@pytest.mark.parametrize("kind,seed", RECIPES)
def test_one_gram_diag_serves_every_rung(kind, seed):
    s = P.recipe(kind, seed)
    _assert_sum_plus_lambda(s.name, s.t_csr_coo(), NL.rungs(s, 32))


@pytest.mark.parametrize("name", ("lambda0_empty_column", "valued"))
def test_one_gram_diag_serves_every_rung_with_lambda_zero(name):
    s = M.systems(large=False)[name]
    lams = [0.0] + NL.rungs(s, 32)
    assert 0.0 in lams and len(set(lams)) >= 32
    _assert_sum_plus_lambda(name, s.t_csr_coo(), lams)
    if name == "lambda0_empty_column":
        d = P.gram_diag(s.t_csr_coo(), 0.0)
        assert d[5] == 0.0 and P.dinv_of(d)[5] == 1.0                # the empty column with lambda = 0: dinv is 1


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed", RECIPES)
def test_every_rung_converges_with_its_own_diagonal(kind, seed):
    s, lams, got = _ladder(kind, seed)
    A = P.dense(s)
    G = A.T @ A
    counts, res = [i.iterations for i in got.infos], []
    for j, lam in enumerate(lams):
        assert got.infos[j].converged == 1, (s.name, j, got.infos[j])
        K = G + lam * np.eye(s.ncol)
        res.append(float(np.linalg.norm(K @ got.X[:, j] - s.b) / np.linalg.norm(s.b)))
        assert res[-1] <= 2 * s.tol, (s.name, j, lam, res[-1])
    print(f"{s.name}: per-column Jacobi counts {counts}, true residuals {min(res) / s.tol:.2f}-{max(res) / s.tol:.2f} tol")
    if kind in ("scaled", "powerlaw"):
        assert len(set(counts)) > 1, (s.name, counts)                # the columns of a ladder freeze at different iterations


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_scaled_ladder_needs_the_columns_own_diagonal(seed):
    s, lams, own = _ladder("scaled", seed)
    t_csr = s.t_csr_coo()
    am, atm, _, _ = M.csr_products(s.nrow, s.ncol, s.a_csr(), t_csr)
    plain = [P.pcg(s.ncol, am, atm, s.b, lam, s.tol, 0) for lam in lams[:7]]
    assert all(c.iterations == s.ncol and c.state["done"] == 0.0 for c in plain), [c.iterations for c in plain]
    shared = P.dinv_of(P.gram_diag(t_csr, min(lams)))
    counts = []
    for j in (5, 6, 7):
        c = P.pcg(s.ncol, am, atm, s.b, lams[j], s.tol, 0, shared)
        counts.append(c.iterations)
        assert c.iterations > 2 * own.infos[j].iterations, (s.name, j, c.iterations, own.infos[j].iterations)
    print(f"{s.name}: shared diagonal {counts} against {[own.infos[j].iterations for j in (5, 6, 7)]} at the three largest rungs")
