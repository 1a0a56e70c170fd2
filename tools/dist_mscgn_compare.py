#!/usr/bin/env python3
"""fs_dist_mscgn -- k targets x m rungs in one solve on the row-sharded matrix -- against fs_mscgn and against what serves the same
k m systems across ranks without it; one process, one GPU, one JSON file.

fs_mscgn's comparison workloads (tools/mscgn_compare.py): config 2's pattern (10 M x 10 M, 16 per row, pattern-only, lambda 5) and
the "control" recipe at nrow x ncol (default 10 M x 1 M, 8 per row, standard normal values, lambda 1e-3); k = 8 targets, the ladder
lambda x {1, 3, 10, 30, 100, 1e3, 1e4, 1e6}, panels in HBM.  Per system:

  one rank      ms per iteration, the slope between caps 8 and 32 at tol 0 (a solve's one-time work taken out), of fs_dist_mscgn on a
                one-rank handle and of fs_mscgn on single-device handles of the same matrix, --repeats interleaved repeats.  One rank
                launches fs_mscgn's kernels and the same two products, so the difference is the host frame.  The bar: the largest
                one-rank ratio profiles/dist_pcgn_lambdas_compare.json records for its own frame (1.022) plus fs_mscgn's own spread
                over its repeats.  The ratio is recorded; outside the bar the JSON says so.
  three ranks   virtual ranks on the one device: host-issue-bound by construction, NOT a scaling result -- the numbers show work and
                exchanges saved.  At tol 1e-8, in both schemes, --repeats interleaved repeats of the wall time of
                  (a) eight solves of fs_dist_mscg, one per target;
                  (b) two solves of fs_dist_pcgn_lambdas with FS_PRECOND_NONE at 32 columns (column 8 r + j of a solve: target j at
                      its rung r; rungs 0-3 in the first solve, 4-7 in the second);
                  (c) ONE fs_dist_mscgn solve;
                each behind one untimed iteration of itself (a solve that follows one of another k re-makes the handle's k-column
                work space, once).  Medians and the spread (max - min) of each, counts and the largest relative residual.
--time-limit S: no further repeat is started once S seconds have passed; the record says how many ran.

Nothing here is a result for more than one real GPU.

    python tools/dist_mscgn_compare.py --what c2,control --out profiles/dist_mscgn_compare.json"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from dist_pcg_compare import PER_ROW, SEED, Sharded, capped_slope, wall  # noqa: E402
from libfastsparse_amd import capi  # noqa: E402

LADDER = (1.0, 3.0, 10.0, 30.0, 100.0, 1e3, 1e4, 1e6)
K = 8
TOL = 1e-8
FRAME_RATIO = 1.022                      # profiles/dist_pcgn_lambdas_compare.json, one rank: 1.0029 (k = 8) .. 1.0216 (k = 32)
VIRTUAL = "virtual ranks, not a scaling result: the one process issues every rank's launches, the ranks share one GPU"
T0 = time.perf_counter()


def med(v):
    return sorted(v)[len(v) // 2]


def stats(v, digits=4):
    return {"all": [round(p, digits) for p in sorted(v)], "median": round(med(v), digits), "spread": round(max(v) - min(v), digits)}


def with_scheme(scheme, f):
    capi.set_option("dist_cg_scheme", scheme)
    try:
        return f()
    finally:
        capi.set_option("dist_cg_scheme", 0)


class Config2:
    """config 2's pattern: single-device handles as tools/mscgn_compare.py makes them, sharded handles as tools/dist_pcg_compare.py"""
    name, lam = "config2", 5.0

    def __init__(self, args):
        self.n = self.ncol = args.n
        self.what = f"config 2 pattern, {self.n} x {self.n}, {PER_ROW} per row, lambda {self.lam}"

    def single(self):
        n = self.n
        rp, cc, _ = capi.synth_uniform(n, n, PER_ROW, SEED, valued=False)
        A = capi.Matrix.from_csr(n, n, rp, cc, None, borrow=True)
        rows = torch.arange(n, device="cuda", dtype=torch.int32).repeat_interleave(PER_ROW)
        At = capi.Matrix.from_coo(n, n, cc, rows, None)
        return A, At, (rp, cc)                                       # (A borrows its arrays: they stay with the handles)

    def sharded(self, ranks):
        return Sharded(self.n, ranks)


class ShardedCsr:
    """equal-length rows as `ranks` row shards from arrays on the device (fs_dist_csr_create_from_shards), A' built on the device"""

    def __init__(self, nrow, ncol, per, cols, vals, ranks):
        L = capi.lib()
        self.D = L.fs_dist_create(ranks, (C.c_int * ranks)(*([0] * ranks)))
        assert self.D, L.fs_last_error()
        cuts = [nrow * r // ranks for r in range(ranks + 1)]
        rps = [torch.arange(0, (cuts[r + 1] - cuts[r]) * per + 1, per, device="cuda", dtype=torch.int32) for r in range(ranks)]
        ccs = [cols[cuts[r] * per:cuts[r + 1] * per].contiguous() for r in range(ranks)]
        vvs = [vals[cuts[r] * per:cuts[r + 1] * per].contiguous() for r in range(ranks)]
        vp = C.c_void_p * ranks
        self.M = L.fs_dist_csr_create_from_shards(self.D, nrow, ncol, (C.c_int * ranks)(*[cuts[r + 1] - cuts[r] for r in range(ranks)]),
                                                  (C.c_int64 * ranks)(*[int(c.numel()) for c in ccs]), vp(*[t.data_ptr() for t in rps]),
                                                  vp(*[t.data_ptr() for t in ccs]), vp(*[t.data_ptr() for t in vvs]), capi.FS_DEVICE)
        assert self.M, L.fs_last_error()
        torch.cuda.synchronize()
        del rps, ccs, vvs
        capi.check(L.fs_dist_matrix_build_transpose_device(self.M), "fs_dist_matrix_build_transpose_device")

    def close(self):
        capi.lib().fs_dist_matrix_destroy(self.M)
        capi.lib().fs_dist_destroy(self.D)


class Control:
    """the "control" recipe of tests/_pcg_model.py at nrow x ncol: one set of arrays behind the single-device and the sharded handles"""
    name, lam, per = "control", 1e-3, 8

    def __init__(self, args):
        self.nrow, self.ncol = args.nrow, args.ncol
        self.what = f"control, {self.nrow} x {self.ncol}, {self.per} per row, standard normal values, lambda {self.lam}"
        g = torch.Generator(device="cuda")
        g.manual_seed(3)
        nnz = self.nrow * self.per
        self.cols = torch.randint(0, self.ncol, (nnz,), device="cuda", dtype=torch.int32, generator=g)
        self.vals = torch.randn(nnz, device="cuda", dtype=torch.float64, generator=g)

    def single(self):
        rows = torch.arange(self.nrow, device="cuda", dtype=torch.int32).repeat_interleave(self.per)
        A = capi.Matrix.from_coo(self.nrow, self.ncol, rows, self.cols, self.vals)
        At = capi.Matrix.from_coo(self.ncol, self.nrow, self.cols, rows, self.vals)
        return A, At, None

    def sharded(self, ranks):
        return ShardedCsr(self.nrow, self.ncol, self.per, self.cols, self.vals, ranks)


def targets(system):
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    return torch.randn((system.ncol, K), device="cuda", dtype=torch.float64, generator=g)


def longest(infos):
    return max((i for row in infos for i in row), key=lambda i: i.iterations)


def one_rank(args, system):
    m = len(LADDER)
    lams = [system.lam * f for f in LADDER]
    A, At, keep = system.single()
    S = system.sharded(1)
    B = targets(system)
    X = torch.empty((m, system.ncol, K), dtype=torch.float64, device="cuda")
    st = capi.current_stream
    counts = {}

    def note(name, cap, infos):
        counts[(name, cap)] = [[i.iterations for i in row] for row in infos]
        return longest(infos)

    solves = {"fs_mscgn": lambda c: note("fs_mscgn", c, capi.mscgn(A, At, X, B, lams, 0.0, max_iter=c, stream=st())),
              "fs_dist_mscgn": lambda c: note("fs_dist_mscgn", c, capi.dist_mscgn(S.M, X, B, lams, 0.0, max_iter=c))}
    for f in solves.values():
        f(3)
    per = {name: [] for name in solves}
    once = {name: [] for name in solves}
    for rep in range(args.repeats):                                  # interleaved, so that drift meets both alike
        if rep and time.perf_counter() - T0 > args.time_limit:
            break
        for name, f in solves.items():
            p, o = capped_slope(f)
            per[name].append(p)
            once[name].append(o)
        print(system.name, "one rank", rep, {k: round(v[-1], 4) for k, v in per.items()}, flush=True)
    rec = {"system": system.what + f"; k {K}, {m} rungs; one rank; slopes between caps 8 and 32 at tol 0", "lambdas": lams,
           "kernels": {"fs_mscgn": [A.kernel_name(), At.kernel_name()]}, "repeats_done": len(per["fs_mscgn"])}
    for name, v in per.items():
        rec[name] = dict(stats(v), one_time_ms=[round(o, 3) for o in sorted(once[name])])
    rec["counts_at_cap_32"] = {name: counts.get((name, 32)) for name in solves}
    rec["same_counts"] = counts.get(("fs_mscgn", 32)) == counts.get(("fs_dist_mscgn", 32))
    base = rec["fs_mscgn"]
    rec["ratio"] = round(rec["fs_dist_mscgn"]["median"] / base["median"], 4)
    rec["bar"] = round(FRAME_RATIO + base["spread"] / base["median"], 4)
    rec["within_bar"] = bool(rec["ratio"] <= rec["bar"])
    if not rec["within_bar"]:
        rec["note"] = "outside the frame's ratio + fs_mscgn's spread: both run the same kernels and products, the difference is the host frame"
    S.close()
    del A, At, keep
    return rec


def three_ranks(args, system):
    m = len(LADDER)
    lams = [system.lam * f for f in LADDER]
    S = system.sharded(3)
    B = targets(system)
    ncol = system.ncol
    cols = [B[:, j].contiguous() for j in range(K)]
    Xa = torch.empty((K, m, ncol), dtype=torch.float64, device="cuda")          # (a): target j, rung i
    Xc = torch.empty((m, ncol, K), dtype=torch.float64, device="cuda")          # (c)
    B32 = B.repeat(1, 4).contiguous()                                           # (b): column 8 r + j is target j
    Xb = torch.empty((2, ncol, 32), dtype=torch.float64, device="cuda")
    lam32 = [[lams[4 * h + c // K] for c in range(32)] for h in (0, 1)]

    def run_a(cap=args.cap):
        return [capi.dist_mscg(S.M, Xa[j], cols[j], lams, TOL, max_iter=cap) for j in range(K)]

    def run_b(cap=args.cap):
        return [capi.dist_pcgn_lambdas(S.M, Xb[h], B32, lam32[h], TOL, max_iter=cap, precond=capi.FS_PRECOND_NONE) for h in (0, 1)]

    def run_c(cap=args.cap):
        return capi.dist_mscgn(S.M, Xc, B, lams, TOL, max_iter=cap)

    names = {"a": "a_eight_solves_of_fs_dist_mscg", "b": "b_two_fs_dist_pcgn_lambdas_at_32_columns", "c": "c_one_fs_dist_mscgn"}
    rec = {"system": system.what + f"; k {K}, {m} rungs, tol {TOL}, cap {args.cap}; three VIRTUAL ranks on one device", "note": VIRTUAL,
           "lambdas": lams}

    def timed(f):
        f(1)                                                         # untimed: the work space of this k and scheme, once
        return wall(f)

    for scheme in (0, 1):
        def both():
            ms = {"a": [], "b": [], "c": []}
            last = {}
            for rep in range(args.repeats):
                if rep and time.perf_counter() - T0 > args.time_limit:
                    break
                for key, f in (("a", run_a), ("b", run_b), ("c", run_c)):
                    last[key], t = timed(f)
                    ms[key].append(t)
                print(system.name, "three ranks scheme", scheme, rep, {k: round(v[-1], 2) for k, v in ms.items()}, flush=True)
            r = {"repeats_done": len(ms["a"])}
            for key, v in ms.items():
                r[names[key]] = {"ms": [round(t, 3) for t in sorted(v)], "median_ms": round(med(v), 3), "spread_ms": round(max(v) - min(v), 3)}
            flat = {"a": [i for row in last["a"] for i in row], "b": [i for row in last["b"] for i in row], "c": [i for row in last["c"] for i in row]}
            for key, infos in flat.items():
                r[names[key]].update(longest_count=max(i.iterations for i in infos), max_relative_residual=max(i.rnorm / i.bnorm for i in infos),
                                     all_converged=all(i.converged for i in infos))
            r[names["c"]]["counts"] = [[i.iterations for i in row] for row in last["c"]]
            # (c) against (a): Xa[j][i] is target j at rung i, Xc[i][:, j] the same system
            r["max_relative_difference_c_to_a"] = max(float((torch.linalg.norm(Xc[i][:, j] - Xa[j][i]) / torch.linalg.norm(Xa[j][i])).item())
                                                      for i in range(m) for j in range(K))
            spread = max(r[n]["spread_ms"] for n in names.values())
            ma, mb, mc = (r[names[k]]["median_ms"] for k in "abc")
            r["largest_spread_ms"] = spread
            r["a_over_c"], r["b_over_c"] = round(ma / mc, 3), round(mb / mc, 3)
            r["c_faster"] = bool(mc + spread < ma and mc + spread < mb)
            return r
        rec[f"scheme{scheme}"] = with_scheme(scheme, both)
    S.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="c2,control")
    ap.add_argument("--parts", default="one,three")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10_000_000, help="rows and columns of config 2's pattern (a rehearsal at a small size says nothing about speed)")
    ap.add_argument("--nrow", type=int, default=10_000_000)
    ap.add_argument("--ncol", type=int, default=1_000_000)
    ap.add_argument("--cap", type=int, default=1000, help="iteration cap of the solves at tol 1e-8")
    ap.add_argument("--time-limit", type=float, default=420.0, help="seconds after which no further repeat is started")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "scope": "one GPU; nothing here is a result for more than one real GPU"}
    if args.out and os.path.exists(args.out):                        # (a run of one system keeps what an earlier run recorded of the other)
        with open(args.out) as fh:
            out.update(json.load(fh))
    for key, cls in (("c2", Config2), ("control", Control)):
        if key not in args.what.split(","):
            continue
        system = cls(args)
        rec = out.setdefault(system.name, {})
        for part, f in (("one", one_rank), ("three", three_ranks)):
            if part in args.parts.split(","):
                rec["one_rank" if part == "one" else "three_virtual_ranks"] = f(args, system)
                if args.out:                                         # (kept after every part: a later part that fails loses nothing)
                    with open(args.out, "w") as fh:
                        json.dump(out, fh, indent=1)
                        fh.write("\n")
        del system
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
