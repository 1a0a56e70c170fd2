"""fs_pcgn on the CPU: its interface and constants are the sources', and the model of its columns (tests/_pcgn_model.py: column j is
the model of fs_pcg on B[:, j]) stays inside fs_pcg's bars on the eight-column recipe.

1  the header declares FS_PCGN_MAX_RHS and fs_pcgn, the binding lists it, the state slots are the sources' and collide with none
   of fs_cg's and fs_pcg's, the key arithmetic lines of the new kernels are in fs_cg.hip;
2  the eight-column recipe (columns scaled by 1e-6 and 1e6, a zero column, the top eigenvector) with Jacobi: every column converges,
   true residual against the dense matrix <= 2 tol (fs_pcg's bar), the counts differ across columns (so freezing is exercised)."""
import os

import numpy as np
import pytest

import _cg_model as M
import _pcg_model as P
import _pcgn_model as N


def _squeezed(*path):
    with open(os.path.join(*path)) as f:
        return " ".join(f.read().split())


def test_interface_and_constants_are_the_sources():
    hdr = _squeezed(M.ROOT, "include", "fastsparse_hip.h")
    assert "enum { FS_PCGN_MAX_RHS = 32 };" in hdr and N.MAX_RHS == 32
    assert ("int fs_pcgn(fs_matrix_t A, fs_matrix_t At, double *X, const double *B, int k, double lambda, const fs_pcg_params *prm, "
            "fs_pcg_info *info /* k entries or NULL */, fs_stream_t stream);") in hdr
    capi = _squeezed(M.ROOT, "libfastsparse_amd", "capi.py")
    assert '"fs_pcgn"' in capi and "def pcgn(A, At, X, B, lam, tol, max_iter=0, precond=" in capi
    got = M.source_constants()
    assert {k: got.get(k) for k in N.PCGN_SOURCE_NAMES} == N.PCGN_SOURCE_NAMES
    assert got["kStDoubles"] == M.CG_STATE_DOUBLES and N.ST_PCGN["live_mask"] < M.CG_STATE_DOUBLES
    new = {"live_mask": N.ST_PCGN["live_mask"]}
    old = set(M.ST1.values()) | set(P.ST_PCG.values())
    assert not set(new.values()) & old                      # the new slot collides with none of fs_cg's and fs_pcg's
    assert sorted(N.PN.values()) == list(range(len(N.PN))) and len(N.PN) <= N.PN_STRIDE
    src = _squeezed(M.CSRC, "fs_cg.hip")
    assert "constexpr int kPcgnMaxRhs = FS_PCGN_MAX_RHS;" in src
    assert 2 * N.MAX_RHS <= M.RED_THREADS                    # one thread per sum, one per column, in the scalar step


def test_arithmetic_is_the_sources():
    """the lines of fs_cg.hip that fs_pcgn's model (fs_pcg's, per column) restates"""
    src = _squeezed(M.CSRC, "fs_cg.hip")
    for line in ("const int cap = prm->max_iter > 0 ? prm->max_iter : F;",
                 # the column steps, each formula written once -- init: cold and warm
                 "if (warm) q = q + l * x; const double r = warm ? b - q : b; bb += b * b; rr += r * r; return r;",
                 # shift-dot
                 "const double q = q0 + l * p; qp += q * p; return q;",
                 # update
                 "double pn_x(double x0, double al, double p) { return x0 + al * p; }",
                 "const double r = r0 - al * q; rr += r * r; return r;",
                 # z of r, direction
                 "if constexpr (std::is_same<CJ, PnOneDiag>::value) return pre ? r * di : r;",
                 "double pn_direction(double z, double be, double p0) { return z + be * p0; }",
                 "double pn_lambda(double lambda, int) { return lambda; }",
                 # the lane-per-row kernels: the steps on the two columns of a pair -- init
                 "const Pair r = {pn_init(warm, q.a, pn_lambda(lambda, c), x.a, b.a, bb[c], rr[c]), "
                 "pn_init(warm, q.b, pn_lambda(lambda, c + 1), x.b, b.b, bb[c + 1], rr[c + 1])};",
                 "if (warm) pn_st<VEC >= 1>(Q + row + c, q, l0, l1); else pn_st<VEC == 2>(X + row + c, {0.0, 0.0}, l0, l1);",
                 # start
                 "const Pair r = v[0][h], z = {pn_z(r.a, dinv != nullptr, di, colj, c), pn_z(r.b, dinv != nullptr, di, colj, c + 1)};",
                 "rz[c] += r.a * z.a; rz[c + 1] += r.b * z.b;",
                 # shift-dot
                 "const Pair q = {pn_shift_dot(q0.a, pn_lambda(lambda, c), p.a, qp[c]), pn_shift_dot(q0.b, pn_lambda(lambda, c + 1), p.b, qp[c + 1])};",
                 # update
                 "const Pair x = {pn_x(x0.a, al[c], p.a), pn_x(x0.b, al[c + 1], p.b)};",
                 "const Pair r = {pn_r(r0.a, al[c], q.a, rr[c]), pn_r(r0.b, al[c + 1], q.b, rr[c + 1])};",
                 "if (sizeof...(LAM) != 0 || dinv) { rz[c] += r.a * pn_z(r.a, dinv != nullptr, di, colj, c); "
                 "rz[c + 1] += r.b * pn_z(r.b, dinv != nullptr, di, colj, c + 1); }",
                 # direction
                 "const Pair p = {pn_direction(z.a, be[c], p0.a), pn_direction(z.b, be[c + 1], p0.b)};",
                 # the same steps on the panels staged through LDS, column by column on the owning thread's row
                 "if (c < k && ((live >> c) & 1u) != 0u) a[c] = col(c, a[c], b[c], di);",
                 "pass(Q, P, nullptr, [&](int c, double q0, double p, double) { return pn_shift_dot(q0, pn_lambda(lam, c), p, qp[c]); });",
                 "if (XUP) pass(X, P, nullptr, [&](int c, double x0, double p, double) { return pn_x(x0, al[c], p); });",
                 "const double r = pn_r(r0, al[c], q, rr[c]); if (sizeof...(LAM) != 0 || dinv) rz[c] += r * pn_z(r, dinv != nullptr, di, colj, c); return r;",
                 "pass(P, R, dinv, [&](int c, double p0, double r, double di) { return pn_direction(pn_z(r, dinv != nullptr, di, colj, c), be[c], p0); });",
                 "for (int blk0 = blockIdx.x * kRedThreads; blk0 < n; blk0 += gridDim.x * kRedThreads)",
                 "for (int row0 = blk0; row0 < blk0 + kRedThreads && row0 < n; row0 += TR) {",
                 "K *const kernel = which == 2 || (which == 0 && k > kPcgnRowsMaxK) ? staged : rows;",
                 # the row a thread owns and where its partial goes
                 "for (int i = blockIdx.x * kRedThreads + threadIdx.x; i < n; i += gridDim.x * kRedThreads) { const size_t row = (size_t)i * k;",
                 "part[(size_t)v * kRedBlocks + blockIdx.x] = s;",
                 "for (int b = threadIdx.x; b < kRedBlocks; b += kRedThreads) a[u] += part[(size_t)v * kRedBlocks + b];",
                 # the scalar steps, per column
                 "const double stop = tol * sqrt(s0); const bool done = sqrt(s1) <= stop;",
                 "e[kPnBb] = s0; e[kPnRr] = s1; e[kPnStop] = stop; e[kPnCount] = 0.0;",
                 "e[kPnLive] = done ? 0.0 : 1.0; e[kPnConverged] = done ? 1.0 : 0.0;",
                 "e[kPnRz] = s0;",
                 "e[kPnAlpha] = e[kPnRz] / s0;",
                 "if (sqrt(rr) <= e[kPnStop]) { e[kPnLive] = 0.0; e[kPnConverged] = 1.0; }",
                 "else { e[kPnBeta] = rz_new / e[kPnRz]; e[kPnRz] = rz_new; e[kPnCount] += 1.0; }",
                 "if (STEP == kPnStepStart) { st[kStIter] = 0.0; st[kStDone] = m ? 0.0 : 1.0; } else if (m == 0u) st[kStDone] = 1.0; else st[kStIter] += 1.0;",
                 # one-time work before anything is written
                 "if (int rc = fs_matrix_prepare(A, k, 0, stream)) return rc; if (int rc = fs_matrix_prepare(At, k, 0, stream)) return rc;"):
        assert line in src, line
    # one copy of each column formula and of each sweep, whatever the kernel, the form and the source of lambda
    for once in ("q0 + l * p", "q + l * x", "x0 + al * p", "r0 - al * q", "z + be * p0", "pn_inv(di,",
                 "i += gridDim.x * kRedThreads) { const size_t row = (size_t)i * k;", "pl_in<KMAX>(t1,", "pl_out<KMAX>("):
        assert src.count(once) == 1, once


@pytest.mark.parametrize("kind", list(N.KIND_ID))
def test_eight_column_recipe_within_the_bars(kind):
    s, B, K = N.recipe8(kind)
    assert B.shape == (s.ncol, 8) and not B[:, 3].any()
    got = N.run(s, B, P.PRECOND_JACOBI)
    counts = [i.iterations for i in got.infos]
    res = []
    for j, info in enumerate(got.infos):
        assert info.converged == 1, (kind, j, info)
        if j == 3:
            assert info.iterations == 0 and M.same_bits(got.X[:, j], np.zeros(s.ncol)).all(), (kind, info)
            continue
        res.append(float(np.linalg.norm(K @ got.X[:, j] - B[:, j]) / np.linalg.norm(B[:, j])))
        assert res[-1] <= 2 * s.tol, (kind, j, res[-1])
        assert info.rnorm <= s.tol * info.bnorm, (kind, j, info)
    print(f"{s.name}: counts {counts}, true residuals {min(res) / s.tol:.2f}-{max(res) / s.tol:.2f} tol")
    assert len(set(counts)) >= 3, counts                      # columns freeze at different iterations
