#!/usr/bin/env python3
"""fs_pcgn against k solves of fs_pcg, one process, one JSON file.

  c2        on config 2's pattern (10 M x 10 M, 16 per row, pattern-only, lambda 5, tol 0 so that no column freezes), without a
            preconditioner and with Jacobi: ms per iteration as the slope between caps 8 and 32 (a solve's one-time work -- work
            space, fs_matrix_prepare, the diagonal, the start, the final copy -- taken out) for fs_pcgn with k = 1, 2, 4, 8, 16, 32
            and for fs_pcg, whose slope times k stands beside every k; repeats interleaved, medians.
            With --kernel-trace, the kernel_trace.csv of a `rocprofv3 --kernel-trace --stats` pass over `pcgn_compare.py --what
            profile` (a run of its own, the program after `--`): the summed median durations of fs_pcgn's own kernels per
            iteration (shift-dot, update, direction, the two scalar steps) at k = 4, 8, 16, 32 against 8 x (12 or 14) x k x F bytes at
            the bandwidth fs_cg's three vector kernels reach in the same trace, times 1.5.  The solves of the profile pass are
            told apart by their order: every fs_pcgn solve starts with one pcgn_init_kernel.  Both variants of the per-iteration
            kernels are traced (option "pcgn_kernel" 1: a lane per row, 2: panels staged through LDS); the solves of c2 run
            with the option at 0, the library's own choice.
  trace     the figures of --kernel-trace alone (no solve runs).
  profile   the solves of that pass: fs_pcg without a preconditioner, then fs_pcgn for every (variant, k, precond) of PROFILE, 12 iterations
            each at tol 0 (every launch does its work).

    python tools/pcgn_compare.py --what c2 --kernel-trace kernel_trace.csv --out profiles/pcgn_compare.json"""
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

# doubles of vector traffic per unknown of fs_cg's three vector kernels
CG_KERNEL_DOUBLES = {"cg_shift_dot_dev_kernel": 3, "cg_update_dev_kernel": 6, "cg_direction_dev_kernel": 3}
PCGN_KERNELS = ("pcgn_shift_dot", "pcgn_update", "pcgn_direction")   # the lane-per-row and the LDS-staged kernels alike
VARIANTS = (("rows", 1), ("lds", 2))                              # option "pcgn_kernel"
KS = (1, 2, 4, 8, 16, 32)
PRECONDS = (("none", capi.FS_PRECOND_NONE, 12), ("jacobi", capi.FS_PRECOND_JACOBI, 14))
PROFILE = [(v, k, p) for v, _ in VARIANTS for k in (4, 8, 16, 32) for p in ("none", "jacobi")]
PROFILE_ITERS = 12
LAM = 5.0
N = 10_000_000                                                  # config 2: rows and columns


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def run_pcg(A, At, x, b, precond, max_iter):
    return wall(lambda: capi.pcg(A, At, x, b, LAM, 0.0, max_iter=max_iter, precond=precond, stream=capi.current_stream()))[1]


def run_pcgn(A, At, X, B, precond, max_iter):
    return wall(lambda: capi.pcgn(A, At, X, B, LAM, 0.0, max_iter=max_iter, precond=precond, stream=capi.current_stream()))[1]


def slope(run, lo=8, hi=32):
    """ms per iteration between caps lo and hi, and what is left of t(lo) as the one-time part"""
    t = {n: run(n) for n in (lo, hi)}
    per = (t[hi] - t[lo]) / (hi - lo)
    return per, t[lo] - lo * per


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def read_trace(path):
    """fs_cg's vector kernels' median ns, and per fs_pcgn solve (in launch order) the median ns of each of its per-iteration
    kernels; the scalar steps are told apart by what they follow (alpha the shift-dot, beta the update).  The median, since
    launches enqueued behind the end of a solve return at once and would pull a mean down"""
    rows = []
    with open(path) as f:
        for row in csv.DictReader(f):
            rows.append((float(row["Start_Timestamp"]), float(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    cg = {k: [] for k in CG_KERNEL_DOUBLES}
    solves, last = [], None
    for t0, t1, name in rows:
        for k in cg:
            if k in name:
                cg[k].append(t1 - t0)
        if "pcgn_init_kernel" in name:
            solves.append({k: [] for k in PCGN_KERNELS + ("step_alpha", "step_beta")})
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
    if not all(cg.values()):
        raise SystemExit(f"{path}: no dispatches of {[k for k, v in cg.items() if not v]}")
    if len(solves) != len(PROFILE):
        raise SystemExit(f"{path}: {len(solves)} fs_pcgn solves, the profile pass runs {len(PROFILE)}")
    return {k: median(v) for k, v in cg.items()}, [{k: median(v) for k, v in s.items()} for s in solves]


def trace_record(path, n):
    """fs_pcgn's own kernels per iteration against their bytes at the bandwidth of fs_cg's vector kernels, both from the trace"""
    cg, solves = read_trace(path)
    gbs = 8.0 * sum(CG_KERNEL_DOUBLES.values()) * n / sum(cg.values())          # bytes per ns
    rec = {"fs_cg_vector_kernels_median_ns": cg, "fs_cg_vector_kernels_GBs": round(gbs, 1)}
    doubles = {name: d for name, _, d in PRECONDS}
    tr = {v: {} for v, _ in VARIANTS}
    for (v, k, p), ns in zip(PROFILE, solves):
        vec = ns["pcgn_shift_dot"] + ns["pcgn_update"] + ns["pcgn_direction"]
        new = vec + ns["step_alpha"] + ns["step_beta"]
        budget = 8.0 * doubles[p] * k * n / gbs
        tr[v][f"k{k}_{p}"] = {"median_ns": ns, "vector_kernels_ms": round(vec * 1e-6, 4), "new_kernels_ms": round(new * 1e-6, 4),
                              "bytes_at_that_bandwidth_ms": round(budget * 1e-6, 4), "ratio": round(new / budget, 3),
                              "vector_kernels_GBs": round(8.0 * doubles[p] * k * n / vec, 1), "within_1.5": bool(new <= 1.5 * budget)}
        print("trace", v, k, p, tr[v][f"k{k}_{p}"], flush=True)
    rec["trace"] = tr                                               # "rows": a lane per row; "lds": the panels staged through LDS
    rec["faster_variant"] = {key: min(tr, key=lambda v: tr[v][key]["new_kernels_ms"]) for key in tr["rows"]}
    rec["new_kernels_within_1.5"] = {key: bool(min(tr[v][key]["ratio"] for v in tr) <= 1.5) for key in tr["rows"]}   # the bar: k = 4, 8, 32
    return rec


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
    x, b = panels[1][0].view(-1), panels[1][1].view(-1)
    by_name = {name: code for name, code, _ in PRECONDS}
    if args.profile:
        print("fs_pcg none", run_pcg(A, At, x, b, capi.FS_PRECOND_NONE, PROFILE_ITERS), flush=True)
        # one-time work first (fs_matrix_prepare measures kernels of its own), so that the traced solves hold iterations only
        for k in sorted({k for _, k, _ in PROFILE}):
            A.prepare(k, capi.current_stream())
            At.prepare(k, capi.current_stream())
        for v, k, p in PROFILE:
            capi.set_option("pcgn_kernel", dict(VARIANTS)[v])
            print("fs_pcgn", v, k, p, run_pcgn(A, At, *panels[k], by_name[p], PROFILE_ITERS), flush=True)
        capi.set_option("pcgn_kernel", 0)
        return
    rec = {"system": "config 2 pattern, 10M x 10M, 16 per row, lambda 5, tol 0, slope between caps 8 and 32; pcgn_kernel 0 (auto)",
           "kernels": [A.kernel_name(), At.kernel_name()], "repeats": args.repeats}
    for name, code, _ in PRECONDS:                                  # warm: the one-time work of every k, every kernel loaded
        run_pcg(A, At, x, b, code, 3)
        for k in KS:
            run_pcgn(A, At, *panels[k], code, 3)
    rec["spmm_plans"] = {str(k): [A.spmm_plan(k), At.spmm_plan(k)] for k in KS if k > 1}
    for name, code, _ in PRECONDS:
        runs = {"fs_pcg": []}
        runs.update({f"fs_pcgn_k{k}": [] for k in KS})
        for _ in range(args.repeats):                               # interleaved, so that drift meets all alike
            runs["fs_pcg"].append(slope(lambda cap: run_pcg(A, At, x, b, code, cap)))
            for k in KS:
                runs[f"fs_pcgn_k{k}"].append(slope(lambda cap: run_pcgn(A, At, *panels[k], code, cap)))
        r = {}
        for key, v in runs.items():
            per = sorted(p for p, _ in v)
            r[key] = {"slope_ms_per_iteration": [round(p, 4) for p in per], "median": round(median(per), 4),
                      "one_time_ms": [round(o, 3) for _, o in sorted(v)]}
        base = r["fs_pcg"]["median"]
        for k in KS:
            e = r[f"fs_pcgn_k{k}"]
            e["k_times_fs_pcg_ms"] = round(k * base, 4)
            e["ratio_to_k_times_fs_pcg"] = round(e["median"] / (k * base), 3)
            print(name, k, e, flush=True)
        rec[name] = r
    if args.kernel_trace:
        rec.update(trace_record(args.kernel_trace, n))
    out["config2"] = rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="c2")
    ap.add_argument("--repeats", type=int, default=3)
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
        out["config2"] = trace_record(args.kernel_trace, N)
    if args.out and not args.profile:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
