#!/usr/bin/env python3
"""fs_mscgn -- k targets x m rungs in one solve -- against what serves the same k m systems without it; one process, one JSON file.

Two systems, both solvable without a preconditioner: config 2's pattern (10 M x 10 M, 16 per row, pattern-only, lambda 5) and the
"control" recipe of tests/_pcg_model.py at nrow x ncol (default 10 M x 1 M, 8 per row, standard normal values, lambda 1e-3).  k = 8
standard normal targets, the ladder lambda x {1, 3, 10, 30, 100, 1e3, 1e4, 1e6}, tol 1e-8.  Per system, --repeats times,
interleaved so that drift meets all alike, the wall time of
  (a) k solves of fs_mscg, one per target;
  (b) two solves of fs_pcgn_lambdas with FS_PRECOND_NONE at 32 columns (column 8 r + j of a solve: target j at its rung r; rungs 0-3
      in the first solve, 4-7 in the second);
  (c) ONE fs_mscgn solve;
medians and the spread (max - min) of each, product pairs, counts, the largest relative residual and the largest relative
difference of (c) to (a).  "c_faster" is true only where the median of (c) is below the medians of (a) and (b) by more than the
largest recorded spread.  Beside that, ms per iteration as the slope between caps 8 and 32 at tol 0 of fs_mscgn and of fs_pcgn at
k = 8 with FS_PRECOND_NONE at the smallest lambda: the price of the shifts.
--time-limit S: no further repeat is started once S seconds have passed; the record says how many ran.

    python tools/mscgn_compare.py --what c2,control --out profiles/mscgn_compare.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from libfastsparse_amd import capi  # noqa: E402

LADDER = (1.0, 3.0, 10.0, 30.0, 100.0, 1e3, 1e4, 1e6)
K = 8
TOL = 1e-8
T0 = time.perf_counter()


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def pairs(infos, cap):
    """product pairs of a solve: the longest recurrence; a converged one ran count + 1"""
    return min(max(i.iterations + i.converged for i in infos), cap)


def med(v):
    return sorted(v)[len(v) // 2]


def compare(args, name, what, A, At, ncol, lam, g):
    m = len(LADDER)
    lams = [lam * f for f in LADDER]
    st = capi.current_stream
    B = torch.randn((ncol, K), device="cuda", dtype=torch.float64, generator=g)
    cols = [B[:, j].contiguous() for j in range(K)]
    Xa = torch.empty((K, m, ncol), dtype=torch.float64, device="cuda")          # (a): target j, rung i
    Xc = torch.empty((m, ncol, K), dtype=torch.float64, device="cuda")          # (c)
    B32 = B.repeat(1, 4).contiguous()                                           # (b): column 8 r + j is target j
    Xb = torch.empty((2, ncol, 32), dtype=torch.float64, device="cuda")
    lam32 = [[lams[4 * h + c // K] for c in range(32)] for h in (0, 1)]
    Xn = torch.empty((ncol, K), dtype=torch.float64, device="cuda")             # fs_pcgn at k = 8

    def run_a(cap=args.cap, tol=TOL):
        return [capi.mscg(A, At, Xa[j], cols[j], lams, tol, max_iter=cap, stream=st()) for j in range(K)]

    def run_b(cap=args.cap, tol=TOL):
        return [capi.pcgn_lambdas(A, At, Xb[h], B32, lam32[h], tol, max_iter=cap, precond=capi.FS_PRECOND_NONE, stream=st()) for h in (0, 1)]

    def run_c(cap=args.cap, tol=TOL):
        return capi.mscgn(A, At, Xc, B, lams, tol, max_iter=cap, stream=st())

    def run_n(cap, tol=0.0):
        return capi.pcgn(A, At, Xn, B, lam, tol, max_iter=cap, precond=capi.FS_PRECOND_NONE, stream=st())

    for f in (run_a, run_b, run_c, run_n):                                      # warm: the one-time work of the products
        f(3)
    rec = {"system": what, "kernels": [A.kernel_name(), At.kernel_name()], "k": K, "lambdas": lams, "tol": TOL, "cap": args.cap}
    ms = {"a": [], "b": [], "c": []}
    slopes = {"fs_mscgn": [], "fs_pcgn_none_k8": []}
    for rep in range(args.repeats):
        if rep and time.perf_counter() - T0 > args.time_limit:
            break
        (ia, ta), (ib, tb), (ic, tc) = wall(run_a), wall(run_b), wall(run_c)
        ms["a"].append(ta)
        ms["b"].append(tb)
        ms["c"].append(tc)
        for key, f in (("fs_mscgn", lambda cap: run_c(cap, 0.0)), ("fs_pcgn_none_k8", run_n)):
            t = {n: wall(lambda: f(n))[1] for n in (8, 32)}
            slopes[key].append((t[32] - t[8]) / 24)
        print(name, rep, {k: round(v[-1], 2) for k, v in ms.items()}, {k: round(v[-1], 3) for k, v in slopes.items()}, flush=True)
    rec["repeats_done"] = len(ms["a"])
    names = {"a": "a_k_solves_of_fs_mscg", "b": "b_two_fs_pcgn_lambdas_at_32_columns", "c": "c_one_fs_mscgn"}
    for key, v in ms.items():
        rec[names[key]] = {"ms": [round(t, 3) for t in sorted(v)], "median_ms": round(med(v), 3), "spread_ms": round(max(v) - min(v), 3)}
    rec[names["a"]].update(product_pairs=sum(pairs(i, args.cap) for i in ia), counts=[[i.iterations for i in row] for row in ia],
                           max_relative_residual=max(i.rnorm / i.bnorm for row in ia for i in row),
                           all_converged=all(i.converged for row in ia for i in row))
    rec[names["b"]].update(product_pairs=sum(pairs(i, args.cap) for i in ib), columns_per_product=32, counts=[[i.iterations for i in row] for row in ib],
                           max_relative_residual=max(i.rnorm / i.bnorm for row in ib for i in row),
                           all_converged=all(i.converged for row in ib for i in row))
    rec[names["c"]].update(product_pairs=pairs([i for row in ic for i in row], args.cap), columns_per_product=K,
                           counts=[[i.iterations for i in row] for row in ic],
                           max_relative_residual=max(i.rnorm / i.bnorm for row in ic for i in row),
                           all_converged=all(i.converged for row in ic for i in row))
    # (c) against (a): Xa[j][i] is target j at rung i, Xc[i][:, j] the same system
    rec["max_relative_difference_c_to_a"] = max(float((torch.linalg.norm(Xc[i][:, j] - Xa[j][i]) / torch.linalg.norm(Xa[j][i])).item())
                                                for i in range(m) for j in range(K))
    spread = max(rec[n]["spread_ms"] for n in names.values())
    ma, mb, mc = (rec[names[k]]["median_ms"] for k in "abc")
    rec["largest_spread_ms"] = spread
    rec["a_over_c"], rec["b_over_c"] = round(ma / mc, 3), round(mb / mc, 3)
    rec["c_faster"] = bool(mc + spread < ma and mc + spread < mb)
    rec["ms_per_iteration_slope_caps_8_32_tol_0"] = {k: {"all": [round(p, 4) for p in sorted(v)], "median": round(med(v), 4)} for k, v in slopes.items()}
    rec["price_of_the_shifts_ms_per_iteration"] = round(med(slopes["fs_mscgn"]) - med(slopes["fs_pcgn_none_k8"]), 4)
    return rec


def config2(args, out):
    n = 10_000_000
    rp, cc, _ = capi.synth_uniform(n, n, 16, 0x5EED0002, valued=False)
    A = capi.Matrix.from_csr(n, n, rp, cc, None, borrow=True)
    rows = torch.arange(n, device="cuda", dtype=torch.int32).repeat_interleave(16)
    At = capi.Matrix.from_coo(n, n, cc, rows, None)                 # A' as its own handle, like the reference's caller
    del rows
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    out["config2"] = compare(args, "config2", "config 2 pattern, 10M x 10M, 16 per row, lambda 5", A, At, n, 5.0, g)


def control(args, out):
    nrow, ncol, per = args.nrow, args.ncol, 8
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    nnz = nrow * per
    rows = torch.arange(nrow, device="cuda", dtype=torch.int32).repeat_interleave(per)
    cols = torch.randint(0, ncol, (nnz,), device="cuda", dtype=torch.int32, generator=g)
    vals = torch.randn(nnz, device="cuda", dtype=torch.float64, generator=g)
    A = capi.Matrix.from_coo(nrow, ncol, rows, cols, vals)
    At = capi.Matrix.from_coo(ncol, nrow, cols, rows, vals)
    del rows, cols, vals
    out["control"] = compare(args, "control", f"control, {nrow} x {ncol}, {per} per row, standard normal values, lambda 0.001", A, At, ncol, 1e-3, g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="c2,control")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=10_000_000)
    ap.add_argument("--ncol", type=int, default=1_000_000)
    ap.add_argument("--cap", type=int, default=1000, help="iteration cap of every timed solve")
    ap.add_argument("--time-limit", type=float, default=420.0, help="seconds after which no further repeat is started")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    what = args.what.split(",")
    out = {"device": torch.cuda.get_device_name(0)}
    if "c2" in what:
        config2(args, out)
    if "control" in what:
        control(args, out)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
