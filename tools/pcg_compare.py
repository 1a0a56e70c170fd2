#!/usr/bin/env python3
"""fs_pcg against fs_cg, one process, one JSON file.

  c2        on config 2's pattern (10 M x 10 M, 16 per row, pattern-only, lambda 5, tol 1e-8): ms per iteration of fs_cg, of fs_pcg
            without a preconditioner and of fs_pcg with Jacobi, five repeats each.  fs_pcg without a preconditioner launches fs_cg's
            kernels, so it has to lie inside the spread of the fs_cg repeats.  Jacobi's extra time per iteration is compared with
            2 * 8 * F bytes at the bandwidth fs_cg's own vector kernels reach, times 1.5 (the second reduction of the update kernel);
            the extra time is given three ways: whole solves, the slope between 8 and 32 iterations (a solve's one-time work --
            work space, the diagonal, the start -- taken out), and the kernels' own durations in the trace;
            that bandwidth comes from --kernel-trace, the kernel_trace.csv of a `rocprofv3 --kernel-trace --stats` pass over
            `pcg_compare.py --what profile` (fs_cg alone).
  scaled    the column-scaled recipe of tests/_pcg_model.py at nrow x ncol (default 10 M x 1 M, 8 per row, lambda 1e-3, tol 1e-8):
            iterations and wall time for no preconditioner (capped at --cap) and for Jacobi.
  powerlaw  the binary power-law recipe (column j with probability ~ 1 / (j + 1), lambda 0.5) at the same size.

    python tools/pcg_compare.py --what c2,scaled,powerlaw --kernel-trace kernel_trace.csv --out profiles/pcg_compare.json"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from libfastsparse_amd import capi  # noqa: E402

# doubles of vector traffic per unknown of fs_cg's three vector kernels
CG_KERNEL_DOUBLES = {"cg_shift_dot_dev_kernel": 3, "cg_update_dev_kernel": 6, "cg_direction_dev_kernel": 3}


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def run_cg(A, At, x, b, lam, tol):
    it = C.c_int(0)
    _, ms = wall(lambda: capi.check(capi.lib().fs_cg(A.h, At.h, x.data_ptr(), b.data_ptr(), lam, tol, C.byref(it), capi.current_stream()), "fs_cg"))
    return {"iterations_run": it.value + 1, "count": it.value, "ms": ms, "ms_per_iteration": ms / (it.value + 1)}


def run_pcg(A, At, x, b, lam, tol, precond, max_iter=0):
    info, ms = wall(lambda: capi.pcg(A, At, x, b, lam, tol, max_iter=max_iter, precond=precond, stream=capi.current_stream()))
    ran = info.iterations + info.converged
    return {"iterations_run": ran, "count": info.iterations, "converged": info.converged, "relative_residual": info.rnorm / info.bnorm,
            "ms": ms, "ms_per_iteration": ms / max(ran, 1)}


def vector_bandwidth(path, F):
    """GB/s of fs_cg's vector kernels from the kernel trace (*_kernel_trace.csv) of the profile pass: their bytes over their median
    durations (the median: launches enqueued behind convergence return at once and would pull a mean down)"""
    ns = {k: [] for k in list(CG_KERNEL_DOUBLES) + ["pcg_update_kernel", "pcg_direction_kernel"]}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in ns:
                if k in row["Kernel_Name"]:
                    ns[k].append(float(row["End_Timestamp"]) - float(row["Start_Timestamp"]))
    if not all(ns.values()):
        raise SystemExit(f"{path}: no dispatches of {[k for k, v in ns.items() if not v]}")
    med = {k: sorted(v)[len(v) // 2] for k, v in ns.items()}
    return 8.0 * sum(CG_KERNEL_DOUBLES.values()) * F / sum(med[k] for k in CG_KERNEL_DOUBLES), med


def slope(A, At, x, b, lam, precond, lo=8, hi=32):
    """ms per iteration with the one-time work of a solve taken out: (t(hi iterations) - t(lo iterations)) / (hi - lo) at tol = 0,
    and what is left of t(lo) as the one-time part (work space, diagonal, start, the final copy)"""
    t = {n: run_pcg(A, At, x, b, lam, 0.0, precond, max_iter=n)["ms"] for n in (lo, hi)}
    per = (t[hi] - t[lo]) / (hi - lo)
    return per, t[lo] - lo * per


def config2(args, out):
    n = 10_000_000
    rp, cc, _ = capi.synth_uniform(n, n, 16, 0x5EED0002, valued=False)
    A = capi.Matrix.from_csr(n, n, rp, cc, None, borrow=True)
    rows = torch.arange(n, device="cuda", dtype=torch.int32).repeat_interleave(16)
    At = capi.Matrix.from_coo(n, n, cc, rows, None)                 # A' as its own handle, like the reference's caller
    del rows
    b = torch.sin(19.0 * torch.arange(n, device="cuda", dtype=torch.float64) + 0.4)
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    lam, tol = 5.0, 1e-8
    if args.profile:
        for _ in range(2):
            print("fs_cg", run_cg(A, At, x, b, lam, tol), flush=True)
        print("fs_pcg jacobi", run_pcg(A, At, x, b, lam, tol, capi.FS_PRECOND_JACOBI), flush=True)
        return
    run_cg(A, At, x, b, lam, tol)                                    # warm
    run_pcg(A, At, x, b, lam, tol, capi.FS_PRECOND_JACOBI)
    rec = {"system": "config 2 pattern, 10M x 10M, 16 per row, lambda 5, tol 1e-8", "kernels": [A.kernel_name(), At.kernel_name()]}
    runs = {"fs_cg": [], "fs_pcg_none": [], "fs_pcg_jacobi": []}
    for _ in range(args.repeats):                                    # interleaved, so that drift meets all three alike
        runs["fs_cg"].append(run_cg(A, At, x, b, lam, tol))
        runs["fs_pcg_none"].append(run_pcg(A, At, x, b, lam, tol, capi.FS_PRECOND_NONE))
        runs["fs_pcg_jacobi"].append(run_pcg(A, At, x, b, lam, tol, capi.FS_PRECOND_JACOBI))
    for k, v in runs.items():
        per = sorted(r["ms_per_iteration"] for r in v)
        rec[k] = {"iterations_run": v[0]["iterations_run"], "ms_per_iteration": [round(p, 4) for p in per], "median": round(per[len(per) // 2], 4)}
        print(k, rec[k], flush=True)
    lo, hi = rec["fs_cg"]["ms_per_iteration"][0], rec["fs_cg"]["ms_per_iteration"][-1]
    rec["none_inside_fs_cg_spread"] = bool(lo <= rec["fs_pcg_none"]["median"] <= hi)
    rec["jacobi_extra_ms_per_iteration"] = round(rec["fs_pcg_jacobi"]["median"] - rec["fs_cg"]["median"], 4)
    # the same with the one-time work of a solve taken out
    sl = {k: sorted(slope(A, At, x, b, lam, p) for _ in range(args.repeats))
          for k, p in (("fs_pcg_none", capi.FS_PRECOND_NONE), ("fs_pcg_jacobi", capi.FS_PRECOND_JACOBI))}
    for k, v in sl.items():
        rec[k]["slope_ms_per_iteration"] = [round(p, 4) for p, _ in v]
        rec[k]["one_time_ms"] = [round(o, 3) for _, o in v]
    rec["jacobi_extra_slope_ms_per_iteration"] = round(sl["fs_pcg_jacobi"][len(sl["fs_pcg_jacobi"]) // 2][0] - sl["fs_pcg_none"][len(sl["fs_pcg_none"]) // 2][0], 4)
    if args.kernel_trace:
        gbs, seen = vector_bandwidth(args.kernel_trace, n)
        rec["vector_kernels_median_ns"] = seen
        rec["fs_cg_vector_kernels_GBs"] = round(gbs, 1)
        rec["jacobi_extra_kernel_ms"] = round((seen["pcg_update_kernel"] - seen["cg_update_dev_kernel"] + seen["pcg_direction_kernel"]
                                               - seen["cg_direction_dev_kernel"]) * 1e-6, 4)
        rec["jacobi_extra_budget_ms"] = round(1.5 * 2 * 8 * n / gbs * 1e-6, 4)     # bytes / (bytes per ns) = ns
        rec["jacobi_extra_within_budget"] = {k: bool(rec[k] <= rec["jacobi_extra_budget_ms"]) for k in
                                             ("jacobi_extra_ms_per_iteration", "jacobi_extra_slope_ms_per_iteration", "jacobi_extra_kernel_ms")}
    out["config2"] = rec


def recipe(args, out, kind):
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
    x = torch.empty(ncol, dtype=torch.float64, device="cuda")
    tol = 1e-8
    run_pcg(A, At, x, b, lam, tol, capi.FS_PRECOND_JACOBI, max_iter=3)   # warm
    rec = {"system": f"{kind}, {nrow} x {ncol}, {per} per row, lambda {lam}, tol {tol}", "kernels": [A.kernel_name(), At.kernel_name()],
           "cap_without_preconditioner": args.cap}
    rec["fs_pcg_jacobi"] = run_pcg(A, At, x, b, lam, tol, capi.FS_PRECOND_JACOBI)
    print(kind, "jacobi", rec["fs_pcg_jacobi"], flush=True)
    rec["fs_pcg_none"] = run_pcg(A, At, x, b, lam, tol, capi.FS_PRECOND_NONE, max_iter=args.cap)
    print(kind, "none", rec["fs_pcg_none"], flush=True)
    out[kind] = rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="c2,scaled,powerlaw")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=10_000_000)
    ap.add_argument("--ncol", type=int, default=1_000_000)
    ap.add_argument("--cap", type=int, default=1000, help="iteration cap of the solves without a preconditioner on the recipes")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    what = args.what.split(",")
    args.profile = "profile" in what
    out = {"device": torch.cuda.get_device_name(0)}
    if args.profile or "c2" in what:
        config2(args, out)
    for kind in ("scaled", "powerlaw"):
        if kind in what:
            recipe(args, out, kind)
    if args.out and not args.profile:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
