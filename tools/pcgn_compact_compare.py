#!/usr/bin/env python3
"""Option "pcgn_compact" (fs_pcgn / fs_pcgn_lambdas move their live columns into narrower panels) against the solve without it; one
process, one JSON file.

  ladder    the two ladders of tools/pcgn_lambdas_compare.py at their sizes (column-scaled and binary power-law, 10 M x 1 M, 8 per
            row, the rungs lambda x {1, 3, 10, 30, 100, 1e3, 1e4, 1e6}, B = b in 8 columns, Jacobi, tol 1e-8): ONE fs_pcgn_lambdas with
            option 0 and with option 1, interleaved, ms per solve as the median of --repeats with the spread, counts, segments, true
            residuals; beside the measured ratio the prediction sum over the iterations of t(width of the iteration) with t(w) =
            fs_pcgn's Jacobi ms per iteration at k = w from profiles/pcgn_compare.json (config 2's pattern: a ratio carries over,
            the milliseconds do not).
  equal     no column finishes early: 8 equal lambdas on config 2's pattern (10 M x 10 M, 16 per row), tol 0, cap 16: option 1 must
            cost nothing beyond the copy of the live mask.
  profile   the solves of the kernel-trace pass, to run under `rocprofv3 --kernel-trace --stats` in a run of its own (the program
            after `--`): the power-law ladder once with option 1.
  trace     from that pass's kernel_trace.csv (--kernel-trace): every pcgn_repack_kernel launch, its ms, the bytes it moves
            (3 (ws + wd) F doubles; ws and wd from the segments the profile run printed, --segments) and bytes/s, next to the
            bytes/s of pcgn_update_lds_kernel at width 8 in the same trace (56 F doubles per launch with Jacobi: X, P, R, Q in, X, R
            out, dinv) -- the project's own streaming yardstick on the same box -- and the ms of one iteration at the width the
            repack leaves (all kernels between two pcgn_shift_dot launches).

A build without the option (the parent commit's library, FS_LIB_PATH) runs `ladder` and `equal` with option 0 alone:
--label parent --out its own file; --parent that file merges its medians into the record.

    python tools/pcgn_compact_compare.py --what ladder,equal --kernel-trace kernel_trace.csv --segments segs.json \\
        --parent parent.json --out profiles/pcgn_compact_compare.json"""
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

LADDER = (1.0, 3.0, 10.0, 30.0, 100.0, 1e3, 1e4, 1e6)
N2 = 10_000_000                                                  # config 2: rows and columns


def has_option():
    return capi.lib().fs_get_option(b"pcgn_compact") >= 0


def set_compact(v):
    if has_option():
        capi.set_option("pcgn_compact", v)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def width_ms():
    """t(w): fs_pcgn's Jacobi ms per iteration at k = w on config 2's pattern, as profiles/pcgn_compare.json has it"""
    with open(os.path.join(ROOT, "profiles", "pcgn_compare.json")) as f:
        rec = json.load(f)["config2"]["jacobi"]
    return {w: rec[f"fs_pcgn_k{w}"]["median"] for w in (1, 2, 4, 8, 16, 32)}


def runs(segments, iterations):
    """(width, iterations at that width) of every segment"""
    ends = [s[0] for s in segments[1:]] + [iterations]
    return [(w, end - first) for (first, w, _), end in zip(segments, ends)]


def predicted(segments, iterations, k, t):
    """sum over the iterations that ran of t(width), and the same at width k throughout"""
    return sum(n * t[w] for w, n in runs(segments, iterations)), iterations * t[k]


def true_residual(A, At, x, b, lam, tmp):
    q = torch.empty_like(x)
    A.spmv(tmp, x, capi.current_stream())
    At.spmv(q, tmp, capi.current_stream())
    return float(torch.linalg.norm(q + lam * x - b) / torch.linalg.norm(b))


def ladder_system(args, kind):
    """the recipes of tools/pcgn_lambdas_compare.py, entry for entry"""
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
    return A, At, b, lam


def compare(args, name, system, A, At, X, B, lams, tol, cap, residuals_of=None):
    """option 0 against option 1 on one solve: --repeats timed solves each, interleaved"""
    st = capi.current_stream()
    k = B.shape[1]
    options = (0, 1) if has_option() else (0,)
    rec = {"system": system, "lambdas": lams, "kernels": [A.kernel_name(), At.kernel_name()], "repeats": args.repeats}
    for o in options:                                             # warm: kernels loaded, the one-time work of every rung's products
        set_compact(o)
        capi.pcgn_lambdas(A, At, X, B, lams, tol, max_iter=3, stream=st)
    ms = {o: [] for o in options}
    last = {}
    for _ in range(args.repeats):
        for o in options:
            set_compact(o)
            infos, t = wall(lambda: capi.pcgn_lambdas(A, At, X, B, lams, tol, max_iter=cap, stream=st))
            ms[o].append(t)
            last[o] = (infos, capi.pcgn_segments() if has_option() else [(0, k, (1 << k) - 1)],
                       residuals_of(X) if residuals_of else None)
    set_compact(0)
    t = width_ms()
    for o in options:
        infos, segs, res = last[o]
        iterations = max(i.iterations + i.converged for i in infos)                          # product pairs that do work
        pred, flat = predicted(segs, iterations, k, t)
        rec[f"option_{o}"] = {"ms": [round(v, 3) for v in ms[o]], "median_ms": round(median(ms[o]), 3),
                              "spread": round((max(ms[o]) - min(ms[o])) / median(ms[o]), 4),
                              "counts": [i.iterations for i in infos], "converged": [i.converged for i in infos],
                              "segments": [list(s) for s in segs], "iterations": iterations,
                              "column_products": sum(w * n for w, n in runs(segs, iterations)),
                              "predicted_config2_ms": round(pred, 2), "predicted_ratio_to_width_k": round(pred / flat, 4)}
        if res is not None:
            rec[f"option_{o}"]["true_residuals"] = res
        print(name, "option", o, rec[f"option_{o}"], flush=True)
    if 1 in options:
        rec["option_1_over_option_0"] = round(rec["option_1"]["median_ms"] / rec["option_0"]["median_ms"], 4)
        rec["option_1_wins"] = bool(rec["option_1"]["median_ms"] < rec["option_0"]["median_ms"])
    return rec


def ladder(args, out, kind):
    A, At, b, lam = ladder_system(args, kind)
    m = len(LADDER)
    lams = [lam * v for v in LADDER]
    tmp = torch.empty(args.nrow, dtype=torch.float64, device="cuda")
    B = b[:, None].repeat(1, m).contiguous()
    X = torch.empty_like(B)
    if args.profile:
        capi.set_option("pcgn_compact", 1)
        capi.pcgn_lambdas(A, At, X, B, lams, 1e-8, max_iter=3, stream=capi.current_stream())   # one-time work outside the traced solve
        torch.cuda.synchronize()
        infos = capi.pcgn_lambdas(A, At, X, B, lams, 1e-8, max_iter=args.cap, stream=capi.current_stream())
        torch.cuda.synchronize()
        out["profile"] = {"ncol": args.ncol, "segments": [list(s) for s in capi.pcgn_segments()], "counts": [i.iterations for i in infos]}
        capi.set_option("pcgn_compact", 0)
        return
    out["ladder_" + kind] = compare(args, kind, f"{kind}, {args.nrow} x {args.ncol}, 8 per row, lambda {lam} x the ladder, tol 1e-8, cap {args.cap}",
                                    A, At, X, B, lams, 1e-8, args.cap,
                                    lambda X_: [true_residual(A, At, X_[:, j].contiguous(), b, lams[j], tmp) for j in range(m)])


def equal(args, out):
    n = N2
    rp, cc, _ = capi.synth_uniform(n, n, 16, 0x5EED0002, valued=False)
    A = capi.Matrix.from_csr(n, n, rp, cc, None, borrow=True)
    rows = torch.arange(n, device="cuda", dtype=torch.int32).repeat_interleave(16)
    At = capi.Matrix.from_coo(n, n, cc, rows, None)
    del rows
    i = torch.arange(n, device="cuda", dtype=torch.float64)
    B = torch.empty((n, 8), dtype=torch.float64, device="cuda")
    for j in range(8):
        B[:, j] = torch.sin((19.0 + j) * i + 0.4 + 0.1 * j)
    del i
    X = torch.empty_like(B)
    out["equal_lambdas_config2"] = compare(args, "equal", "config 2 pattern, 10M x 10M, 16 per row, 8 equal lambdas (5.0), Jacobi, tol 0, cap 16: "
                                           "no column finishes early", A, At, X, B, [5.0] * 8, 0.0, 16)


def trace_record(path, seg_path):
    """every repack launch against the update kernel of the same trace, and against one iteration at the width it leaves"""
    with open(seg_path) as f:
        prof = json.load(f)["profile"]
    F, segs = prof["ncol"], prof["segments"]
    rows = []
    with open(path) as f:
        for row in csv.DictReader(f):
            rows.append((float(row["Start_Timestamp"]), float(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    inits = [i for i, r in enumerate(rows) if "pcgn_init_kernel" in r[2]]
    rows = rows[inits[-1]:]                                        # the traced solve: behind the last start
    # a repack is pcgn_repack_kernel with pcgn_remap_kernel right behind it (the way back of finished columns runs ahead of it)
    packs = [(i, r) for i, r in enumerate(rows[:-1]) if "pcgn_repack_kernel" in r[2] and "pcgn_remap_kernel" in rows[i + 1][2]]
    upd = [r[1] - r[0] for r in rows[:packs[0][0]] if "pcgn_update_lds_kernel" in r[2]] if packs else []
    out = {"F": F, "segments": segs, "repacks": []}
    if upd:
        ns = median(upd)
        out["pcgn_update_lds_kernel_width_8"] = {"median_ms": round(ns * 1e-6, 4), "bytes": 56 * F * 8,
                                                 "GBs": round(56 * F * 8 / ns, 1)}
    dots = [i for i, r in enumerate(rows) if "pcgn_shift_dot" in r[2]]
    for (i, r), (prev, seg) in zip(packs, zip(segs[:-1], segs[1:])):
        ws, wd = prev[1], seg[1]
        ns = r[1] - r[0]
        after = [d for d in dots if d > i]
        it = rows[after[1]][0] - rows[after[0]][0] if len(after) > 1 else None      # one iteration at the width the repack leaves
        # (the products run ahead of the shift-dot: from one shift-dot's start to the next's is one whole iteration)
        e = {"at_iteration": seg[0], "from_width": ws, "to_width": wd, "ms": round(ns * 1e-6, 4), "bytes": 3 * (ws + wd) * F * 8,
             "GBs": round(3 * (ws + wd) * F * 8 / ns, 1), "one_iteration_at_to_width_ms": None if it is None else round(it * 1e-6, 4)}
        if it is not None:
            e["repack_costs_less_than_that_iteration"] = bool(ns < it)
        out["repacks"].append(e)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="ladder,equal")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nrow", type=int, default=10_000_000)
    ap.add_argument("--ncol", type=int, default=1_000_000)
    ap.add_argument("--cap", type=int, default=1000)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--segments", default=None, help="the JSON the profile run wrote (--out of --what profile)")
    ap.add_argument("--parent", default=None, help="the JSON of a run on the parent commit's library (--label parent)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    what = args.what.split(",")
    args.profile = "profile" in what
    out = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "label": args.label,
           "has_option_pcgn_compact": has_option()}
    if args.profile:
        ladder(args, out, "powerlaw")
    else:
        if "ladder" in what:
            for kind in ("scaled", "powerlaw"):
                ladder(args, out, kind)
        if "equal" in what:
            equal(args, out)
        if args.kernel_trace and args.segments:
            out["kernel_trace_powerlaw_option_1"] = trace_record(args.kernel_trace, args.segments)
        if args.parent:
            with open(args.parent) as f:
                parent = json.load(f)
            out["parent_commit_option_0"] = {}
            for key, rec in parent.items():
                if isinstance(rec, dict) and "option_0" in rec and key in out:
                    mine, theirs = out[key]["option_0"], rec["option_0"]
                    margin = max(mine["spread"], theirs["spread"])
                    ratio = mine["median_ms"] / theirs["median_ms"]
                    out["parent_commit_option_0"][key] = {"parent_ms": theirs["ms"], "parent_median_ms": theirs["median_ms"],
                                                          "this_build_median_ms": mine["median_ms"], "ratio": round(ratio, 4),
                                                          "margin_run_to_run_spread": round(margin, 4),
                                                          "equal_within_the_spread": bool(abs(ratio - 1.0) <= margin)}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
