#!/usr/bin/env python3
"""What the shifts of a multi-shift solve cost on the sharded path, against what they cost on one device: one GPU, one JSON file.

On config 2's pattern (10 M x 10 M, 16 per row, pattern-only, lambda 5), vectors in HBM, the m = 8 ladder lambda * {1, 3, 10, 30, 100,
1e3, 1e4, 1e6} (tests/_mscg_model.py LADDER), tol 0, ms per iteration as the slope between caps 8 and 32 (a solve's one-time work taken
out), --repeats interleaved repeats of everything, the spread (max - min over the repeats) of every slope recorded:

  --what single   fs_mscg and fs_pcg without a preconditioner on single-device handles: S_single = fs_mscg - fs_pcg.  Meant for the
                  PARENT commit's build (--package-root names its checkout: its libfastsparse_amd package and library are used), so
                  that the figure is what the shifts cost before fs_mscg moved onto the launchers it now shares with fs_dist_mscg.
  --what dist     fs_dist_mscg and fs_dist_pcg without a preconditioner on one rank, at this commit: S_dist = fs_dist_mscg -
                  fs_dist_pcg.  The same kernels on the same data as `single`: the expected difference is zero.  With --single-from
                  (the JSON of a `single` run of the same session) the bar is evaluated:
                      S_dist <= S_single + 2 x the largest of the four recorded spreads
                  (a difference of differences carries two spreads on each side).
  --what three    three VIRTUAL ranks on the one device, both schemes, recorded without a bar: the ranks share one GPU and one issuing
                  thread, so this is NOT a scaling result.  RCCL with more than one rank has never run this code.

    python tools/dist_mscg_compare.py --what single --package-root <parent checkout> --label "parent commit <hash>" --out single.json
    python tools/dist_mscg_compare.py --what dist,three --single-from single.json --out profiles/dist_mscg_compare.json"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, PER_ROW, SEED, LAM = 10_000_000, 16, 0x5EED0002, 5.0
LADDER = (1.0, 3.0, 10.0, 30.0, 100.0, 1e3, 1e4, 1e6)                # tests/_mscg_model.py LADDER
LAMS = [LAM * f for f in LADDER]
torch = capi = None


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


class Sharded:
    """config 2's pattern as `ranks` row shards generated on the device (fs_dist_csr_create_from_shards), A' built on the device"""

    def __init__(self, n, ranks):
        L = capi.lib()
        self.D = L.fs_dist_create(ranks, (C.c_int * ranks)(*([0] * ranks)))
        assert self.D, L.fs_last_error()
        cuts = [n * r // ranks for r in range(ranks + 1)]
        shards = [capi.synth_uniform(cuts[r + 1] - cuts[r], n, PER_ROW, SEED, row_offset=cuts[r], valued=False) for r in range(ranks)]
        rows = (C.c_int * ranks)(*[cuts[r + 1] - cuts[r] for r in range(ranks)])
        nnz = (C.c_int64 * ranks)(*[int(s[1].numel()) for s in shards])
        rps = (C.c_void_p * ranks)(*[s[0].data_ptr() for s in shards])
        ccs = (C.c_void_p * ranks)(*[s[1].data_ptr() for s in shards])
        self.M = L.fs_dist_csr_create_from_shards(self.D, n, n, rows, nnz, rps, ccs, None, capi.FS_DEVICE)
        assert self.M, L.fs_last_error()
        del shards
        capi.check(L.fs_dist_matrix_build_transpose_device(self.M), "fs_dist_matrix_build_transpose_device")

    def close(self):
        capi.lib().fs_dist_matrix_destroy(self.M)
        capi.lib().fs_dist_destroy(self.D)


def capped_slope(solve, lo=8, hi=32):
    """ms per iteration between two solves at tol 0 whose base system runs exactly lo and hi iterations"""
    t = {}
    for n in (lo, hi):
        info, t[n] = wall(lambda: solve(n))
        assert info.iterations == n and info.converged == 0, (n, info.iterations, info.converged)
    return (t[hi] - t[lo]) / (hi - lo)


def measure(solves, repeats):
    """{name: {ms_per_iteration (sorted), median, spread_ms}}: one warm solve each, then `repeats` interleaved rounds"""
    for f in solves.values():
        f(3)
    per = {k: [] for k in solves}
    for _ in range(repeats):                                         # interleaved, so that drift meets all of them alike
        for k, f in solves.items():
            per[k].append(capped_slope(f))
    rec = {}
    for k, v in per.items():
        v = sorted(v)
        rec[k] = {"ms_per_iteration": [round(p, 4) for p in v], "median": round(v[len(v) // 2], 4), "spread_ms": round(v[-1] - v[0], 4)}
        print(k, rec[k], flush=True)
    return rec


def vectors(n):
    b = torch.sin(19.0 * torch.arange(n, device="cuda", dtype=torch.float64) + 0.4)
    return b, torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty((len(LAMS), n), dtype=torch.float64, device="cuda")


def single(args, out):
    n = args.n
    rp, cc, _ = capi.synth_uniform(n, n, PER_ROW, SEED, valued=False)
    A = capi.Matrix.from_csr(n, n, rp, cc, None, borrow=True)
    rows = torch.arange(n, device="cuda", dtype=torch.int32).repeat_interleave(PER_ROW)
    At = capi.Matrix.from_coo(n, n, cc, rows, None)
    del rows
    b, x, X = vectors(n)
    st = capi.current_stream()
    rec = measure({"fs_pcg_none": lambda c: capi.pcg(A, At, x, b, LAM, 0.0, max_iter=c, precond=capi.FS_PRECOND_NONE, stream=st),
                   "fs_mscg_m8": lambda c: capi.mscg(A, At, X, b, LAMS, 0.0, max_iter=c, stream=st)[0]}, args.repeats)
    rec["system"] = f"config 2 pattern, {n} x {n}, {PER_ROW} per row, lambda {LAM} * {list(LADDER)}; single-device handles; slopes between caps 8 and 32 at tol 0"
    rec["build"] = args.label
    rec["kernels"] = [A.kernel_name(), At.kernel_name()]
    rec["S_single_ms"] = round(rec["fs_mscg_m8"]["median"] - rec["fs_pcg_none"]["median"], 4)
    out["single_device"] = rec


def dist(args, out):
    n = args.n
    S = Sharded(n, 1)
    b, x, X = vectors(n)
    rec = measure({"fs_dist_pcg_none": lambda c: capi.dist_pcg(S.M, x, b, LAM, 0.0, max_iter=c, precond=capi.FS_PRECOND_NONE),
                   "fs_dist_mscg_m8": lambda c: capi.dist_mscg(S.M, X, b, LAMS, 0.0, max_iter=c)[0]}, args.repeats)
    rec["system"] = f"config 2 pattern, {n} x {n}, {PER_ROW} per row, lambda {LAM} * {list(LADDER)}; one rank; slopes between caps 8 and 32 at tol 0"
    rec["S_dist_ms"] = round(rec["fs_dist_mscg_m8"]["median"] - rec["fs_dist_pcg_none"]["median"], 4)
    out["one_rank"] = rec
    S.close()


def three(args, out):
    n = args.n
    S = Sharded(n, 3)
    b, x, X = vectors(n)
    solves = {}
    for scheme in (0, 1):
        def with_scheme(f, scheme=scheme):
            def run(c):
                capi.set_option("dist_cg_scheme", scheme)
                try:
                    return f(c)
                finally:
                    capi.set_option("dist_cg_scheme", 0)
            return run
        solves[f"scheme{scheme}_fs_dist_pcg_none"] = with_scheme(lambda c: capi.dist_pcg(S.M, x, b, LAM, 0.0, max_iter=c, precond=capi.FS_PRECOND_NONE))
        solves[f"scheme{scheme}_fs_dist_mscg_m8"] = with_scheme(lambda c: capi.dist_mscg(S.M, X, b, LAMS, 0.0, max_iter=c)[0])
    rec = measure(solves, args.repeats)
    rec["system"] = f"config 2 pattern, {n} x {n}, {PER_ROW} per row, lambda {LAM} * {list(LADDER)}; three VIRTUAL ranks on one device"
    rec["note"] = ("virtual ranks, not a scaling result: the one process issues every rank's launches, the ranks share one GPU; no figure for "
                   "real multi-GPU hardware exists, RCCL with more than one rank has never run this code")
    out["three_virtual_ranks"] = rec
    S.close()


def bar(out):
    """S_dist against S_single + 2 x the largest of the four spreads"""
    one, sd = out["one_rank"], out["single_device"]
    spreads = {"fs_dist_mscg_m8": one["fs_dist_mscg_m8"]["spread_ms"], "fs_dist_pcg_none": one["fs_dist_pcg_none"]["spread_ms"],
               "fs_mscg_m8": sd["fs_mscg_m8"]["spread_ms"], "fs_pcg_none": sd["fs_pcg_none"]["spread_ms"]}
    allowance = 2 * max(spreads.values())
    out["shift_cost"] = {"S_dist_ms": one["S_dist_ms"], "S_single_ms": sd["S_single_ms"], "spreads_ms": spreads,
                         "allowance_ms": round(allowance, 4), "bar": "S_dist <= S_single + 2 x the largest of the four spreads",
                         "met": bool(one["S_dist_ms"] <= sd["S_single_ms"] + allowance)}
    print("shift_cost", out["shift_cost"], flush=True)


def main():
    global torch, capi
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="dist,three")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=N, help="rows and columns (a rehearsal at a small size says nothing about speed)")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose libfastsparse_amd package and library are measured")
    ap.add_argument("--label", default="this commit", help="what --package-root holds, for the record (e.g. the parent commit's hash)")
    ap.add_argument("--single-from", default=None, help="the JSON of a --what single run: its record is copied and the bar evaluated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch as _torch
    from libfastsparse_amd import capi as _capi
    torch, capi = _torch, _capi
    out = {"device": torch.cuda.get_device_name(0)}
    what = args.what.split(",")
    if "single" in what:
        single(args, out)
    if args.single_from:
        with open(args.single_from) as f:
            out["single_device"] = json.load(f)["single_device"]
    if "dist" in what:
        dist(args, out)
    if "three" in what:
        three(args, out)
    if "one_rank" in out and "single_device" in out:
        bar(out)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
