#!/usr/bin/env python3
"""fs_mscg against fs_cg / fs_pcg, one process, one JSON file.

  c2        on config 2's pattern (10 M x 10 M, 16 per row, pattern-only, lambda 5 + 0.01 i, tol 0 so that no shift freezes): ms per
            iteration as the slope between caps 8 and 32 (a solve's one-time work -- work space, start, final copy -- taken out), for
            fs_mscg with m = 1, 2, 4, 8, 16 and, as the capped baseline, for fs_pcg without a preconditioner (key
            "fs_pcg_none_capped": it launches fs_cg's kernels and takes a cap, but it is NOT fs_cg: its last step is another step of
            final_step_kernel, kStepPcgBeta), five repeats each, interleaved.  fs_cg ITSELF takes no cap, so its ms per iteration (key "fs_cg")
            is the slope between two of its own solves that stop at tol 1e-3 and 1e-8, (t2 - t1) / (count2 - count1).  m = 1 runs
            fs_cg's vector traffic plus two one-workgroup launches: its difference to fs_cg, and to the capped baseline, is given
            beside the spread of the fs_cg repeats.  The cost per extra shift,
            (t(m = 8) - t(m = 1)) / 7, is compared with 5 F * 8 bytes at the bandwidth fs_cg's own three vector kernels reach, times
            1.5 (the margin tools/pcg_compare.py grants its fused kernel; here it stands for the many concurrent streams).  That
            bandwidth comes from --kernel-trace, the kernel_trace.csv of a `rocprofv3 --kernel-trace --stats` pass over
            `mscg_compare.py --what profile` (a run of its own, the program after `--`).
  powerlaw  the binary power-law recipe of tests/_pcg_model.py (column j with probability ~ 1 / (j + 1), lambda 0.5) at nrow x ncol
            (default 10 M x 1 M, 8 per row) with the ladder lambda * {1, 3, 10, 30, 100, 1e3, 1e4, 1e6} at tol 1e-8: wall time and
            product pairs of ONE fs_mscg against eight fs_pcg solves without a preconditioner, every solve under the same --cap.

    python tools/mscg_compare.py --what c2,powerlaw --kernel-trace kernel_trace.csv --out profiles/mscg_compare.json"""
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
LADDER = (1.0, 3.0, 10.0, 30.0, 100.0, 1e3, 1e4, 1e6)
SHIFTS = (1, 2, 4, 8, 16)
PROFILE_M = 8


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def run_pcg(A, At, x, b, lam, tol, max_iter):
    info, ms = wall(lambda: capi.pcg(A, At, x, b, lam, tol, max_iter=max_iter, precond=capi.FS_PRECOND_NONE, stream=capi.current_stream()))
    return info, ms


def run_cg(A, At, x, b, lam, tol):
    it = C.c_int(0)
    _, ms = wall(lambda: capi.check(capi.lib().fs_cg(A.h, At.h, x.data_ptr(), b.data_ptr(), lam, tol, C.byref(it), capi.current_stream()), "fs_cg"))
    return it.value, ms


def cg_slope(A, At, x, b, lam, tols=(1e-3, 1e-8)):
    """fs_cg itself takes no cap: ms per iteration between two of its solves that stop at different tolerances"""
    (n1, t1), (n2, t2) = (run_cg(A, At, x, b, lam, tol) for tol in tols)
    per = (t2 - t1) / (n2 - n1)
    return per, t1 - (n1 + 1) * per, (n1, n2)


def run_mscg(A, At, X, b, lams, tol, max_iter):
    infos, ms = wall(lambda: capi.mscg(A, At, X, b, lams, tol, max_iter=max_iter, stream=capi.current_stream()))
    return infos, ms


def slope(run, lo=8, hi=32):
    """ms per iteration between caps lo and hi, and what is left of t(lo) as the one-time part"""
    t = {n: run(n) for n in (lo, hi)}
    per = (t[hi] - t[lo]) / (hi - lo)
    return per, t[lo] - lo * per


def trace_medians(path, names):
    """median duration in ns of every kernel of `names` in a rocprofv3 kernel trace (*_kernel_trace.csv); the median, since
    launches enqueued behind the end of a solve return at once and would pull a mean down"""
    ns = {k: [] for k in names}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in ns:
                if k in row["Kernel_Name"]:
                    ns[k].append(float(row["End_Timestamp"]) - float(row["Start_Timestamp"]))
    if not all(ns.values()):
        raise SystemExit(f"{path}: no dispatches of {[k for k, v in ns.items() if not v]}")
    return {k: sorted(v)[len(v) // 2] for k, v in ns.items()}


def config2(args, out):
    n = 10_000_000
    rp, cc, _ = capi.synth_uniform(n, n, 16, 0x5EED0002, valued=False)
    A = capi.Matrix.from_csr(n, n, rp, cc, None, borrow=True)
    rows = torch.arange(n, device="cuda", dtype=torch.int32).repeat_interleave(16)
    At = capi.Matrix.from_coo(n, n, cc, rows, None)                 # A' as its own handle, like the reference's caller
    del rows
    b = torch.sin(19.0 * torch.arange(n, device="cuda", dtype=torch.float64) + 0.4)
    X = torch.empty((max(SHIFTS), n), dtype=torch.float64, device="cuda")
    lams = [5.0 + 0.01 * i for i in range(max(SHIFTS))]
    if args.profile:                                                # tol 0, 12 iterations each: every launch does its work
        print("fs_pcg none", run_pcg(A, At, X[0], b, lams[0], 0.0, 12)[1], flush=True)
        print("fs_mscg", PROFILE_M, run_mscg(A, At, X[:PROFILE_M], b, lams[:PROFILE_M], 0.0, 12)[1], flush=True)
        return
    run_pcg(A, At, X[0], b, lams[0], 0.0, 3)                         # warm
    run_mscg(A, At, X, b, lams, 0.0, 3)
    run_cg(A, At, X[0], b, lams[0], 1e-3)
    rec = {"system": "config 2 pattern, 10M x 10M, 16 per row, lambda 5 + 0.01 i, tol 0, slope between caps 8 and 32",
           "kernels": [A.kernel_name(), At.kernel_name()]}
    runs = {"fs_cg": [], "fs_pcg_none_capped": []}
    runs.update({f"fs_mscg_m{m}": [] for m in SHIFTS})
    for _ in range(args.repeats):                                    # interleaved, so that drift meets all alike
        per, once, rec["fs_cg_counts_at_tol_1e-3_1e-8"] = cg_slope(A, At, X[0], b, lams[0])
        runs["fs_cg"].append((per, once))
        runs["fs_pcg_none_capped"].append(slope(lambda cap: run_pcg(A, At, X[0], b, lams[0], 0.0, cap)[1]))
        for m in SHIFTS:
            runs[f"fs_mscg_m{m}"].append(slope(lambda cap: run_mscg(A, At, X[:m], b, lams[:m], 0.0, cap)[1]))
    med = {}
    for k, v in runs.items():
        per = sorted(p for p, _ in v)
        med[k] = per[len(per) // 2]
        rec[k] = {"slope_ms_per_iteration": [round(p, 4) for p in per], "median": round(med[k], 4),
                  "one_time_ms": [round(o, 3) for _, o in sorted(v)]}
        print(k, rec[k], flush=True)
    cg = rec["fs_cg"]["slope_ms_per_iteration"]
    rec["m1_minus_fs_cg_ms"] = round(med["fs_mscg_m1"] - med["fs_cg"], 4)
    rec["m1_minus_fs_pcg_none_capped_ms"] = round(med["fs_mscg_m1"] - med["fs_pcg_none_capped"], 4)
    rec["fs_cg_spread_ms"] = round(cg[-1] - cg[0], 4)
    rec["per_extra_shift_ms"] = round((med["fs_mscg_m8"] - med["fs_mscg_m1"]) / 7, 4)
    rec["per_extra_shift_ms_m16"] = round((med["fs_mscg_m16"] - med["fs_mscg_m1"]) / 15, 4)
    if args.kernel_trace:
        seen = trace_medians(args.kernel_trace, list(CG_KERNEL_DOUBLES) + ["mscg_update_kernel", "mscg_direction_kernel"])
        gbs = 8.0 * sum(CG_KERNEL_DOUBLES.values()) * n / sum(seen[k] for k in CG_KERNEL_DOUBLES)   # bytes per ns
        rec["vector_kernels_median_ns"] = seen
        rec["fs_cg_vector_kernels_GBs"] = round(gbs, 1)
        rec["per_extra_shift_at_that_bandwidth_ms"] = round(5 * 8 * n / gbs * 1e-6, 4)
        rec["per_extra_shift_ratio"] = round(rec["per_extra_shift_ms"] / rec["per_extra_shift_at_that_bandwidth_ms"], 3)
        rec["per_extra_shift_within_1.5"] = bool(rec["per_extra_shift_ratio"] <= 1.5)
        # the two kernels' own durations in the trace (m = PROFILE_M, 7 live shifts) over fs_cg's, per shift
        extra = seen["mscg_update_kernel"] - seen["cg_update_dev_kernel"] + seen["mscg_direction_kernel"] - seen["cg_direction_dev_kernel"]
        rec["per_extra_shift_kernel_ms"] = round(extra / (PROFILE_M - 1) * 1e-6, 4)
        rec["mscg_vector_kernels_GBs"] = round(8.0 * (9 + 5 * (PROFILE_M - 1)) * n / (seen["mscg_update_kernel"] + seen["mscg_direction_kernel"]), 1)
    out["config2"] = rec


def powerlaw(args, out):
    nrow, ncol, per = args.nrow, args.ncol, 8
    g = torch.Generator(device="cuda")
    g.manual_seed(2)
    nnz = nrow * per
    rows = torch.arange(nrow, device="cuda", dtype=torch.int32).repeat_interleave(per)
    cdf = torch.cumsum(1.0 / torch.arange(1, ncol + 1, device="cuda", dtype=torch.float64), 0)
    u = torch.rand(nnz, device="cuda", dtype=torch.float64, generator=g) * cdf[-1]
    cols = torch.searchsorted(cdf, u).clamp_(max=ncol - 1).to(torch.int32)
    del u, cdf
    lam, tol = 0.5, 1e-8
    A = capi.Matrix.from_coo(nrow, ncol, rows, cols, None)
    At = capi.Matrix.from_coo(ncol, nrow, cols, rows, None)
    del rows, cols
    b = torch.randn(ncol, device="cuda", dtype=torch.float64, generator=g)
    lams = [lam * f for f in LADDER]
    X = torch.empty((len(lams), ncol), dtype=torch.float64, device="cuda")
    Y = torch.empty((len(lams), ncol), dtype=torch.float64, device="cuda")
    run_pcg(A, At, Y[0], b, lam, tol, 3)                             # warm
    run_mscg(A, At, X, b, lams, tol, 3)
    rec = {"system": f"powerlaw, {nrow} x {ncol}, {per} per row, lambda 0.5 * {list(LADDER)}, tol {tol}, cap {args.cap}",
           "kernels": [A.kernel_name(), At.kernel_name()]}
    infos, ms = run_mscg(A, At, X, b, lams, tol, args.cap)
    pairs = max(i.iterations + i.converged for i in infos)           # the base runs longest; a converged solve ran count + 1
    rec["fs_mscg"] = {"ms": round(ms, 3), "product_pairs": min(pairs, args.cap), "counts": [i.iterations for i in infos],
                      "converged": [i.converged for i in infos], "relative_residuals": [i.rnorm / i.bnorm for i in infos]}
    print("fs_mscg", rec["fs_mscg"], flush=True)
    sep = [run_pcg(A, At, Y[i], b, l, tol, args.cap) for i, l in enumerate(lams)]
    rec["fs_pcg_each"] = {"ms": [round(t, 3) for _, t in sep], "ms_together": round(sum(t for _, t in sep), 3),
                          "product_pairs": sum(min(i.iterations + i.converged, args.cap) for i, _ in sep),
                          "counts": [i.iterations for i, _ in sep], "converged": [i.converged for i, _ in sep],
                          "relative_residuals": [i.rnorm / i.bnorm for i, _ in sep]}
    print("fs_pcg each", rec["fs_pcg_each"], flush=True)
    rec["max_relative_difference"] = [float((torch.linalg.norm(X[i] - Y[i]) / torch.linalg.norm(Y[i])).item()) for i in range(len(lams))]
    rec["speedup"] = round(rec["fs_pcg_each"]["ms_together"] / ms, 3)
    rec["product_pairs_ratio"] = round(rec["fs_pcg_each"]["product_pairs"] / max(rec["fs_mscg"]["product_pairs"], 1), 3)
    rec["fs_mscg_faster_than_the_eight"] = bool(ms < rec["fs_pcg_each"]["ms_together"])
    out["powerlaw"] = rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="c2,powerlaw")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=10_000_000)
    ap.add_argument("--ncol", type=int, default=1_000_000)
    ap.add_argument("--cap", type=int, default=1000, help="iteration cap of every solve on the recipe")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    what = args.what.split(",")
    args.profile = "profile" in what
    out = {"device": torch.cuda.get_device_name(0)}
    if args.profile or "c2" in what:
        config2(args, out)
    if "powerlaw" in what:
        powerlaw(args, out)
    if args.out and not args.profile:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
