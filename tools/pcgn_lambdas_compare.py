#!/usr/bin/env python3
"""fs_pcgn_lambdas against fs_pcgn, and a ladder of lambdas in one solve against eight fs_pcg solves and one fs_mscg; one process, one
JSON file.

  c2        on config 2's pattern (10 M x 10 M, 16 per row, pattern-only, tol 0 so that no column freezes), without a preconditioner and
            with Jacobi: ms per iteration as the slope between caps 8 and 32, and what is left of t(8) as the one-time part per solve
            (work space, the diagonal, the start, the final copy; fs_pcgn_lambdas has one fs_gram_diag and no pass that inverts it), for
            fs_pcgn at lambda 5 and fs_pcgn_lambdas at k distinct lambdas (5 x the ladder), k = 4, 8, 16, 32; repeats interleaved,
            medians.  With --kernel-trace, the kernel_trace.csv of a `rocprofv3 --kernel-trace --stats` pass over
            `pcgn_lambdas_compare.py --what profile` (a run of its own, no counters, the program after `--`): the summed median
            durations per iteration of the vector kernels and the two scalar steps of both solvers, at k = 4, 8, 16, 32 and in both
            forms of the kernels (option "pcgn_kernel" 1: a lane per row, 2: panels staged through LDS).  The bytes of the two solvers
            are the same, so with Jacobi any excess of fs_pcgn_lambdas is its division per element: the budget is 16 / 14 of
            fs_pcgn's figure at the same k and form, what a stored F x k panel of inverse diagonals would cost in traffic.  Without a
            preconditioner only the lambda operand differs: the budget is the spread of fs_pcgn's own repeats in the same trace.
  trace     the figures of --kernel-trace alone (no solve runs).
  profile   the solves of that pass: for every (form, k, precond) fs_pcgn and fs_pcgn_lambdas in turn, PROFILE_REPEATS times, 12
            iterations each at tol 0 (every launch does its work).  The solves are told apart by their order: each starts with one
            pcgn_init_kernel.
  ladder    the column-scaled and the binary power-law recipe of tools/pcg_compare.py (10 M x 1 M, 8 per row) with the rungs
            lambda x {1, 3, 10, 30, 100, 1e3, 1e4, 1e6} at tol 1e-8, cap 1000: ONE fs_pcgn_lambdas (B = b in 8 columns, Jacobi)
            against eight fs_pcg Jacobi solves and against ONE fs_mscg: total ms, product pairs, per-rung counts and true residuals;
            the one solve again with its 8-column products as single-vector sweeps (option "spmm_kernel" 3).

    python tools/pcgn_lambdas_compare.py --what c2,ladder --kernel-trace kernel_trace.csv --out profiles/pcgn_lambdas_compare.json"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from libfastsparse_amd import capi  # noqa: E402

PCGN_KERNELS = ("pcgn_shift_dot", "pcgn_update", "pcgn_direction")   # the lane-per-row and the LDS-staged kernels alike
VARIANTS = (("rows", 1), ("lds", 2))                              # option "pcgn_kernel"
KS = (4, 8, 16, 32)
PRECONDS = (("none", capi.FS_PRECOND_NONE), ("jacobi", capi.FS_PRECOND_JACOBI))
SOLVERS = ("fs_pcgn", "fs_pcgn_lambdas")
PROFILE_REPEATS = 3
PROFILE = [(v, k, p, s, r) for v, _ in VARIANTS for k in KS for p, _ in PRECONDS for r in range(PROFILE_REPEATS) for s in SOLVERS]
PROFILE_ITERS = 12
LAM = 5.0
LADDER = (1.0, 3.0, 10.0, 30.0, 100.0, 1e3, 1e4, 1e6)
N = 10_000_000                                                  # config 2: rows and columns
JACOBI_BUDGET = 16.0 / 14.0


def rungs(lam, k):
    return [lam * LADDER[j % 8] * (1.0 + 0.25 * (j // 8)) for j in range(k)]


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def run(solver, A, At, X, B, precond, max_iter):
    st = capi.current_stream()
    if solver == "fs_pcgn":
        return wall(lambda: capi.pcgn(A, At, X, B, LAM, 0.0, max_iter=max_iter, precond=precond, stream=st))[1]
    return wall(lambda: capi.pcgn_lambdas(A, At, X, B, rungs(LAM, B.shape[1]), 0.0, max_iter=max_iter, precond=precond, stream=st))[1]


def slope(f, lo=8, hi=32):
    """ms per iteration between caps lo and hi, and what is left of t(lo) as the one-time part"""
    t = {n: f(n) for n in (lo, hi)}
    per = (t[hi] - t[lo]) / (hi - lo)
    return per, t[lo] - lo * per


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def read_trace(path):
    """per solve of the profile pass (in launch order) the median ns of each of its per-iteration kernels; the scalar steps are told
    apart by what they follow (alpha the shift-dot, beta the update).  The median, since launches enqueued behind the end of a solve
    return at once and would pull a mean down"""
    rows = []
    with open(path) as f:
        for row in csv.DictReader(f):
            rows.append((float(row["Start_Timestamp"]), float(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    solves, last = [], None
    for t0, t1, name in rows:
        if "pcgn_init_kernel" in name:
            solves.append({k: [] for k in PCGN_KERNELS + ("step_alpha", "step_beta")})
            solves[-1]["per_column"] = "PcgnLambdas" in name
            last = None
        if not solves:
            continue
        if "pcgn_step_kernel" in name:
            if last in ("pcgn_shift_dot", "pcgn_update"):
                solves[-1]["step_alpha" if last == "pcgn_shift_dot" else "step_beta"].append(t1 - t0)
            last = None
        for k in PCGN_KERNELS:
            if k in name:
                solves[-1][k].append(t1 - t0)
                last = k
    if len(solves) != len(PROFILE):
        raise SystemExit(f"{path}: {len(solves)} solves, the profile pass runs {len(PROFILE)}")
    for (_, _, _, s, _), got in zip(PROFILE, solves):
        if got.pop("per_column") != (s == "fs_pcgn_lambdas"):
            raise SystemExit(f"{path}: the solves are not in the order of the profile pass")
    return [{k: median(v) for k, v in s.items()} for s in solves]


def trace_record(path):
    """the kernels of fs_pcgn_lambdas per iteration against fs_pcgn's, same trace, and the budgets"""
    per = {}
    for (v, k, p, s, _), ns in zip(PROFILE, read_trace(path)):
        per.setdefault((v, k, p), {}).setdefault(s, []).append(ns)
    tr = {v: {} for v, _ in VARIANTS}
    for (v, k, p), by in per.items():
        e = {}
        for s in SOLVERS:
            tot = [sum(ns.values()) for ns in by[s]]
            e[s] = {"kernels_ms": [round(t * 1e-6, 4) for t in tot], "median_ms": round(median(tot) * 1e-6, 4),
                    "median_ns_by_kernel": by[s][tot.index(median(tot))]}
        base, spread = e["fs_pcgn"]["median_ms"], (max(e["fs_pcgn"]["kernels_ms"]) - min(e["fs_pcgn"]["kernels_ms"])) / e["fs_pcgn"]["median_ms"]
        e["ratio"] = round(e["fs_pcgn_lambdas"]["median_ms"] / base, 4)
        e["fs_pcgn_spread"] = round(spread, 4)
        e["budget"] = round(JACOBI_BUDGET, 4) if p == "jacobi" else round(1.0 + spread, 4)
        e["within_budget"] = bool(e["ratio"] <= e["budget"])
        tr[v][f"k{k}_{p}"] = e
        print("trace", v, k, p, e["fs_pcgn"]["kernels_ms"], e["fs_pcgn_lambdas"]["kernels_ms"], "ratio", e["ratio"], "budget", e["budget"], flush=True)
    return {"trace": tr,                                            # "rows": a lane per row; "lds": the panels staged through LDS
            "within_budget": {v: {key: e["within_budget"] for key, e in tr[v].items()} for v in tr}}


def config2(args, out):
    n = N
    rp, cc, _ = capi.synth_uniform(n, n, 16, 0x5EED0002, valued=False)
    A = capi.Matrix.from_csr(n, n, rp, cc, None, borrow=True)
    rows = torch.arange(n, device="cuda", dtype=torch.int32).repeat_interleave(16)
    At = capi.Matrix.from_coo(n, n, cc, rows, None)                 # A' as its own handle, like the reference's caller
    del rows
    i = torch.arange(n, device="cuda", dtype=torch.float64)
    kmax = max(KS)
    B = torch.empty((n, kmax), dtype=torch.float64, device="cuda")
    for j in range(kmax):                                           # distinct columns, all of the scale of config 2's b
        B[:, j] = torch.sin((19.0 + j) * i + 0.4 + 0.1 * j)
    del i
    panels = {k: (torch.empty((n, k), dtype=torch.float64, device="cuda"), B[:, :k].contiguous()) for k in KS}
    by_name = dict(PRECONDS)
    if args.profile:
        # one-time work first (fs_matrix_prepare measures kernels of its own), so that the traced solves hold iterations only
        for k in KS:
            A.prepare(k, capi.current_stream())
            At.prepare(k, capi.current_stream())
        for v, k, p, s, _ in PROFILE:
            capi.set_option("pcgn_kernel", dict(VARIANTS)[v])
            print(s, v, k, p, run(s, A, At, *panels[k], by_name[p], PROFILE_ITERS), flush=True)
        capi.set_option("pcgn_kernel", 0)
        return
    rec = {"system": "config 2 pattern, 10M x 10M, 16 per row, tol 0, slope between caps 8 and 32; pcgn_kernel 0 (auto); fs_pcgn at "
                     "lambda 5, fs_pcgn_lambdas at 5 x the ladder",
           "kernels": [A.kernel_name(), At.kernel_name()], "repeats": args.repeats}
    for _, code in PRECONDS:                                        # warm: the one-time work of every k, every kernel loaded
        for k in KS:
            for s in SOLVERS:
                run(s, A, At, *panels[k], code, 3)
    for name, code in PRECONDS:
        runs = {(s, k): [] for s in SOLVERS for k in KS}
        for _ in range(args.repeats):                               # interleaved, so that drift meets all alike
            for k in KS:
                for s in SOLVERS:
                    runs[s, k].append(slope(lambda cap: run(s, A, At, *panels[k], code, cap)))
        r = {}
        for k in KS:
            e = {}
            for s in SOLVERS:
                per = sorted(p for p, _ in runs[s, k])
                once = sorted(o for _, o in runs[s, k])
                e[s] = {"slope_ms_per_iteration": [round(p, 4) for p in per], "median": round(median(per), 4),
                        "one_time_ms": [round(o, 3) for o in once], "one_time_median_ms": round(median(once), 3)}
            e["ratio"] = round(e["fs_pcgn_lambdas"]["median"] / e["fs_pcgn"]["median"], 4)
            r[f"k{k}"] = e
            print(name, k, e, flush=True)
        rec[name] = r
    if args.kernel_trace:
        rec.update(trace_record(args.kernel_trace))
    out["config2"] = rec


def true_residual(A, At, x, b, lam, tmp):
    q = torch.empty_like(x)
    A.spmv(tmp, x, capi.current_stream())
    At.spmv(q, tmp, capi.current_stream())
    return float(torch.linalg.norm(q + lam * x - b) / torch.linalg.norm(b))


def ladder(args, out, kind):
    nrow, ncol, per = args.nrow, args.ncol, 8
    g = torch.Generator(device="cuda")
    g.manual_seed(1 if kind == "scaled" else 2)
    nnz = nrow * per
    rows = torch.arange(nrow, device="cuda", dtype=torch.int32).repeat_interleave(per)
    if kind == "powerlaw":
        cdf = torch.cumsum(1.0 / torch.arange(1, ncol + 1, device="cuda", dtype=torch.float64), 0)
        u = torch.rand(nnz, device="cuda", dtype=torch.float64, generator=g) * cdf[-1]
        cols = torch.searchsorted(cdf, u).clamp_(max=ncol - 1).to(torch.int32)
        del u, cdf
        vals, lam = None, 0.5
    else:
        cols = torch.randint(0, ncol, (nnz,), device="cuda", dtype=torch.int32, generator=g)
        scale = 10.0 ** (torch.rand(ncol, device="cuda", dtype=torch.float64, generator=g) * 3.0 - 1.5)
        vals = torch.randn(nnz, device="cuda", dtype=torch.float64, generator=g) * scale[cols.long()]
        lam = 1e-3
    A = capi.Matrix.from_coo(nrow, ncol, rows, cols, vals)
    At = capi.Matrix.from_coo(ncol, nrow, cols, rows, vals)
    del rows, cols, vals
    b = torch.randn(ncol, device="cuda", dtype=torch.float64, generator=g)
    tol, m = 1e-8, len(LADDER)
    lams = rungs(lam, m)
    st = capi.current_stream()
    x, tmp = torch.empty(ncol, dtype=torch.float64, device="cuda"), torch.empty(nrow, dtype=torch.float64, device="cuda")
    B = b[:, None].repeat(1, m).contiguous()
    X, Xm = torch.empty_like(B), torch.empty((m, ncol), dtype=torch.float64, device="cuda")
    capi.pcg(A, At, x, b, lams[0], tol, max_iter=3, stream=st)      # warm: kernels loaded, the one-time work of the 8-column products
    capi.pcgn_lambdas(A, At, X, B, lams, tol, max_iter=3, stream=st)
    capi.mscg(A, At, Xm, b, lams, tol, max_iter=3, stream=st)
    rec = {"system": f"{kind}, {nrow} x {ncol}, {per} per row, lambda {lam} x the ladder, tol {tol}, cap {args.cap}", "lambdas": lams,
           "kernels": [A.kernel_name(), At.kernel_name()], "spmm_plans_k8": [A.spmm_plan(m), At.spmm_plan(m)]}

    def entry(infos, ms, xs, pairs):
        return {"ms": round(ms, 3), "product_pairs": pairs, "counts": [i.iterations for i in infos], "converged": [i.converged for i in infos],
                "true_residuals": [true_residual(A, At, xs(j), b, lams[j], tmp) for j in range(m)]}

    infos, ms = wall(lambda: capi.pcgn_lambdas(A, At, X, B, lams, tol, max_iter=args.cap, stream=st))
    rec["one_fs_pcgn_lambdas"] = entry(infos, ms, lambda j: X[:, j].contiguous(), max(i.iterations + i.converged for i in infos))
    print(kind, "fs_pcgn_lambdas", rec["one_fs_pcgn_lambdas"], flush=True)
    # the same solve with the 8-column products as one single-vector sweep per column (option "spmm_kernel" 3): what the solve
    # costs where the k-column plan of a heavy-tailed A' is the slow part
    capi.set_option("spmm_kernel", 3)
    try:
        capi.pcgn_lambdas(A, At, X, B, lams, tol, max_iter=3, stream=st)
        infos, ms = wall(lambda: capi.pcgn_lambdas(A, At, X, B, lams, tol, max_iter=args.cap, stream=st))
        rec["one_fs_pcgn_lambdas_spmm_kernel_3"] = entry(infos, ms, lambda j: X[:, j].contiguous(), max(i.iterations + i.converged for i in infos))
    except RuntimeError as e:
        rec["one_fs_pcgn_lambdas_spmm_kernel_3"] = {"error": str(e)}
    finally:
        capi.set_option("spmm_kernel", 0)
    print(kind, "fs_pcgn_lambdas, spmm_kernel 3", rec["one_fs_pcgn_lambdas_spmm_kernel_3"], flush=True)
    xs, each, total = [], [], 0.0
    for lam_j in lams:
        info, ms = wall(lambda: capi.pcg(A, At, x, b, lam_j, tol, max_iter=args.cap, stream=st))
        xs.append(x.clone())
        each.append(info)
        total += ms
    rec["eight_fs_pcg_jacobi"] = entry(each, total, lambda j: xs[j], sum(i.iterations + i.converged for i in each))
    print(kind, "eight fs_pcg", rec["eight_fs_pcg_jacobi"], flush=True)
    del xs
    infos, ms = wall(lambda: capi.mscg(A, At, Xm, b, lams, tol, max_iter=args.cap, stream=st))
    rec["one_fs_mscg"] = entry(infos, ms, lambda j: Xm[j].contiguous(), max(i.iterations + i.converged for i in infos))
    print(kind, "fs_mscg", rec["one_fs_mscg"], flush=True)
    rec["one_solve_over_eight"] = round(rec["one_fs_pcgn_lambdas"]["ms"] / rec["eight_fs_pcg_jacobi"]["ms"], 3)
    out["ladder_" + kind] = rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="c2,ladder")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nrow", type=int, default=10_000_000)
    ap.add_argument("--ncol", type=int, default=1_000_000)
    ap.add_argument("--cap", type=int, default=1000, help="iteration cap of the solves on the ladder")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    what = args.what.split(",")
    args.profile = "profile" in what
    out = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None}
    if args.profile or "c2" in what:
        config2(args, out)
    elif "trace" in what:
        if not args.kernel_trace:
            raise SystemExit("--what trace needs --kernel-trace")                                           # the trace's figures alone, from an earlier profile pass
        out["config2"] = trace_record(args.kernel_trace)
    if "ladder" in what and not args.profile:
        for kind in ("scaled", "powerlaw"):
            ladder(args, out, kind)
    if args.out and not args.profile:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
