"""The device as a backend of tests/_truth.py: one draw of make_case through one solver's entry point, on the harness of tests/_gpu.py,
_solvers.py and _dist_solvers.py (helper; no test in here).  tests/test_gpu_fuzz_solvers.py runs a fixed seeded stretch through it,
tools/fuzz_solvers.py an open-ended one.

A solve gets its buffers from Case.buffers (guards, gaps, a start), the case's options around the creation of the handles and around
the call, and comes back as a _truth.Result; the relations the header states between solvers are run here too, on variants of the
case (one column of it, one shift of it, another option)."""
import contextlib
import copy
import ctypes as C

import numpy as np

import _cg_model as M
import _dist_solvers as DSV
import _truth as T
from _gpu import mode_options, options


@contextlib.contextmanager
def scope(L, case, handle=None, **over):
    """the case's options: its mode, pcgn_kernel, pcgn_compact, dist_cg_scheme (over: other values for a relation's second solve).
    Mode "spmv_kernel" forces a kernel: the code of the copy the handle keeps where it keeps one, else 2, a wave's lanes per row"""
    opts = dict(pcgn_kernel=case.pcgn_kernel, pcgn_compact=case.pcgn_compact, dist_cg_scheme=case.scheme)
    mode = over.pop("mode", case.mode)
    opts.update(over)
    with contextlib.ExitStack() as stack:
        if mode == "spmv_kernel":
            kept = L.fs_matrix_spmv_kernel(handle, 0) if handle else 0
            stack.enter_context(options(reproducible=0, spmv_kernel=kept if kept >= 6 else 2))
        else:
            stack.enter_context(mode_options(mode))
        stack.enter_context(options(**opts))
        yield


def system_of(case):
    return M.System(f"draw{case.draw}", case.nrow, case.F, case.rows, case.cols, case.vals, case.B[:, 0], None, case.lam, case.tol)


class Single:
    """A and A' of a case on one device: from COO, A' in the caller's entry order; or (sorted_t) from the CSR of A and the sorted A'
    that the shards of a built transpose hold"""

    def __init__(self, L, case, sorted_t=False, mode=None):
        from libfastsparse_amd import capi
        from _gpu import to_device
        self.L, self.ranks = L, 0
        with scope(L, case, **({} if mode is None else {"mode": mode})):
            if sorted_t:
                import _solvers as SV
                self.A, self.At = SV.single_handles(L, system_of(case))
            else:
                vals = None if case.vals is None else to_device(case.vals)
                self.A = capi.Matrix.from_coo(case.nrow, case.F, to_device(case.rows), to_device(case.cols), vals)
                self.At = capi.Matrix.from_coo(case.F, case.nrow, to_device(case.cols), to_device(case.rows), vals)
        self.handle = self.A.h

    def close(self):
        self.A.close()
        self.At.close()


class Sharded:
    """the case on `ranks` virtual ranks of device 0, A' built from the host arrays or on the device"""

    def __init__(self, L, case, ranks, mode=None):
        self.L, self.ranks, self.handle = L, ranks, None
        with scope(L, case, **({} if mode is None else {"mode": mode})):
            self.dist = DSV.Dist(L, system_of(case), ranks, case.device_t)

    def close(self):
        self.dist.close()


def open_for(L, case, solver, ranks=None):
    return Sharded(L, case, case.ranks if ranks is None else ranks) if solver.startswith("dist_") else Single(L, case)


def solve(L, h, case, solver, cap, tol, hbm=True, **over):
    """one call of the solver's entry point: (status, X's buffer, B's buffer, the m k infos)"""
    import torch
    from libfastsparse_amd import capi
    m, k = case.shape(solver)
    xoff, ldx, _, boff, _ = case.layout(solver)
    xbuf, bbuf = case.buffers(solver)
    diag = case.diag_of(solver)
    if hbm:
        xd, bd = torch.from_numpy(xbuf).cuda(), torch.from_numpy(bbuf).cuda()
        dd = None if diag is None else torch.from_numpy(np.ascontiguousarray(diag)).cuda()
        xp, bp, dp = xd.data_ptr() + 8 * xoff, bd.data_ptr() + 8 * boff, None if dd is None else dd.data_ptr()
    else:
        dd = None if diag is None else np.ascontiguousarray(diag)
        xp, bp, dp = xbuf.ctypes.data + 8 * xoff, bbuf.ctypes.data + 8 * boff, None if dd is None else dd.ctypes.data
    prm = capi.PcgParams(float(tol), int(cap), int(case.precond) if T.preconditioned(solver) else 0, int(case.warm(solver)), dp)
    infos = (capi.PcgInfo * (m * k))()
    lams = case.lams(solver)
    fam, sharded = T.family(solver), solver.startswith("dist_")
    lam_k = (C.c_double * k)(*[float(v) for v in lams[0]])
    lam_m = (C.c_double * m)(*[float(v) for v in lams[:, 0]])
    stream = None if sharded else capi.current_stream()
    with scope(L, case, h.handle, **over):
        if not sharded:
            A, At = h.A.h, h.At.h
            if fam == "pcg":
                rc = L.fs_pcg(A, At, xp, bp, float(case.lam), C.byref(prm), infos, stream)
            elif fam == "pcgn":
                rc = L.fs_pcgn(A, At, xp, bp, k, float(case.lam), C.byref(prm), infos, stream)
            elif fam == "pcgn_lambdas":
                rc = L.fs_pcgn_lambdas(A, At, xp, bp, k, lam_k, C.byref(prm), infos, stream)
            elif fam == "mscg":
                rc = L.fs_mscg(A, At, xp, ldx, bp, m, lam_m, float(tol), int(cap), infos, stream)
            else:
                rc = L.fs_mscgn(A, At, xp, ldx, bp, k, m, lam_m, float(tol), int(cap), infos, stream)
        else:
            Mh = h.dist.M
            if fam == "pcg":
                rc = L.fs_dist_pcg(Mh, xp, bp, float(case.lam), C.byref(prm), infos)
            elif fam == "pcgn":
                rc = L.fs_dist_pcgn(Mh, xp, bp, k, float(case.lam), C.byref(prm), infos)
            elif fam == "pcgn_lambdas":
                rc = L.fs_dist_pcgn_lambdas(Mh, xp, bp, k, lam_k, C.byref(prm), infos)
            elif fam == "mscg":
                rc = L.fs_dist_mscg(Mh, xp, ldx, bp, m, lam_m, float(tol), int(cap), infos)
            else:
                rc = L.fs_dist_mscgn(Mh, xp, ldx, bp, k, m, lam_m, float(tol), int(cap), infos)
    if hbm:
        torch.cuda.synchronize()
        xbuf, bbuf = xd.cpu().numpy(), bd.cpu().numpy()
    return rc, xbuf, bbuf, [T.Info(int(g.iterations), int(g.converged), float(g.rnorm), float(g.bnorm)) for g in infos]


def run(L, h, case, solver):
    """the case's two solves, the one that runs to F twice: two _truth.Result.  The sharded solvers take their vectors from host
    memory on odd draws, from HBM on even ones"""
    hbm = not solver.startswith("dist_") or case.draw % 2 == 0
    out = []
    for n, (cap, tol) in enumerate(case.solves()):
        rc, xbuf, bbuf, infos = solve(L, h, case, solver, cap, tol, hbm)
        again = None
        if n == 0 and rc == T.FS_OK:
            _, xbuf2, _, infos2 = solve(L, h, case, solver, cap, tol, hbm)
            again = (xbuf2, infos2)
        out.append(T.Result(solver, cap, tol, rc, xbuf, bbuf, infos, again))
    return out


def run_and_check(L, case, solver, ranks=None):
    """open the handles, run the case's solves, hold each against the truth: what check() returns, per solve"""
    h = open_for(L, case, solver, ranks)
    try:
        return [T.check(case, r) for r in run(L, h, case, solver)]
    finally:
        h.close()


# ---- the relations the header states ---------------------------------------------------------------------------------------
def variant(case, X0=None, **fields):
    """the case with other fields (a column of it, a shift of it, ...); X0: {solver: its warm start}, so that a variant starts where
    the column it stands for started"""
    v = copy.copy(case)
    v._x0, v._refs, v._twins = dict(X0 or {}), {}, []
    for name, value in fields.items():
        setattr(v, name, value)
    return v


def column_of(case, solver, j, single):
    """column j of a panel solve as a case of the single-vector solver `single`"""
    X0 = case.X0(solver)
    lam = float(case.lams(solver)[0, j])
    return variant(case, {single: None if X0 is None else np.ascontiguousarray(X0[:, [j]])}, B=np.ascontiguousarray(case.B[:, [j]]), k=1,
                   lam=lam, lams_k=[lam])


def _x(case, solver, out):
    return case.X_of(solver, out[1]), out[3]


def relations(L, case):
    """the header's statements that tie two solvers or two options together, on the cases they apply to; bit for bit, X and infos.
    Returns how many pairs of solves were compared.  A case whose mode is cg_fixed_order = 0 promises no bits and runs none."""
    if case.mode == "cg_fixed_order=0":
        return 0
    cap, tol = case.solves()[case.draw % 2]                                     # the full solve on even draws, the capped one on odd ones
    strict = case.mode == "strict_order"
    k, m = case.k, case.m
    some = sorted({0, k - 1, k // 2})                                           # the columns a relation looks at
    done = 0
    h = Single(L, case)
    try:
        def go(c, solver, **over):
            rc, xbuf, _, infos = solve(L, h, c, solver, cap, tol, True, **over)
            assert rc == T.FS_OK, (repr(c), solver, rc)
            return c.X_of(solver, xbuf), infos

        base = {s: go(case, s) for s in ("pcgn", "pcgn_lambdas", "mscgn")}
        if strict:
            for solver in ("pcgn", "pcgn_lambdas"):                             # column j IS fs_pcg on B[:, j] at lambda[j]
                X, infos = base[solver]
                for j in some:
                    x1, i1 = go(column_of(case, solver, j, "pcg"), "pcg")
                    T.same_pair((repr(case), solver, j, "is fs_pcg"), X[0, :, j], infos[j], x1[0, :, 0], i1[0])
                    done += 1
                Xc, ic = go(case, solver, pcgn_compact=1 - case.pcgn_compact)   # pcgn_compact = 1 has the bits of 0
                for j in range(k):
                    T.same_pair((repr(case), solver, j, "pcgn_compact"), X[0, :, j], infos[j], Xc[0, :, j], ic[j])
                done += 1
            X, infos = base["mscgn"]                                            # column j of fs_mscgn IS fs_mscg on B[:, j]
            for j in some:
                c1 = variant(case, B=np.ascontiguousarray(case.B[:, [j]]), k=1)
                x1, i1 = go(c1, "mscg")
                for i in range(m):
                    T.same_pair((repr(case), "mscgn", (i, j), "is fs_mscg"), X[i, :, j], infos[i * k + j], x1[i, :, 0], i1[i])
                done += 1
        for solver in ("pcgn", "pcgn_lambdas", "mscgn"):                        # the two pcgn_kernel forms agree
            X, infos = go(case, solver, pcgn_kernel=1)
            X2, infos2 = go(case, solver, pcgn_kernel=2)
            for n in range(len(infos)):
                i, j = divmod(n, k)
                T.same_pair((repr(case), solver, (i, j), "pcgn_kernel 1 and 2"), X[i, :, j], infos[n], X2[i, :, j], infos2[n])
            done += 1
        # m = 1 of fs_mscgn is fs_pcgn with no preconditioner from a cold start
        lam0 = float(case.ladder[0])
        Xm, im = go(variant(case, m=1, ladder=[lam0]), "mscgn")
        Xp, ip = go(variant(case, lam=lam0, precond=T.NONE, start="cold"), "pcgn", pcgn_compact=0)
        for j in range(k):
            T.same_pair((repr(case), "mscgn m = 1 is pcgn", j), Xm[0, :, j], im[j], Xp[0, :, j], ip[j])
        done += 1
        # k = 1 of each panel solver is its single-vector solver, in every mode
        for panel, single in (("pcgn", "pcg"), ("pcgn_lambdas", "pcg"), ("mscgn", "mscg")):
            if panel == "mscgn":
                c1 = variant(case, B=np.ascontiguousarray(case.B[:, [0]]), k=1)
            else:
                c1 = column_of(case, panel, 0, single)
                c1._x0[panel] = c1._x0[single]
            Xa, ia = go(c1, panel)
            Xb, ib = go(c1, single)
            for i in range(len(ia)):
                T.same_pair((repr(case), panel, "k = 1 is", single, i), Xa[i, :, 0], ia[i], Xb[i, :, 0], ib[i])
            done += 1
    finally:
        h.close()
    if strict:                                                                  # dist_cg_scheme 0 on virtual ranks IS the single-device solver
        hs, hd = Single(L, case, sorted_t=True), Sharded(L, case, case.ranks)
        try:
            for solver in T.SOLVERS[:5]:
                rc, xbuf, _, infos = solve(L, hs, case, solver, cap, tol, True)
                rc2, xbuf2, _, infos2 = solve(L, hd, case, "dist_" + solver, cap, tol, True, dist_cg_scheme=0)
                assert rc == T.FS_OK and rc2 == T.FS_OK, (repr(case), solver, rc, rc2)
                X, X2 = case.X_of(solver, xbuf), case.X_of(solver, xbuf2)
                kk = case.shape(solver)[1]
                for n in range(len(infos)):
                    i, j = divmod(n, kk)
                    T.same_pair((repr(case), "dist_" + solver, (i, j), "scheme 0 is the single-device solver"), X[i, :, j], infos[n], X2[i, :, j], infos2[n])
                done += 1
        finally:
            hs.close()
            hd.close()
    return done
