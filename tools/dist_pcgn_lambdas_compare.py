#!/usr/bin/env python3
"""fs_dist_pcgn_lambdas against fs_dist_pcgn and against itself in the other scheme, one process, one GPU, one JSON file.

On config 2's pattern (10 M x 10 M, 16 per row, pattern-only, lambda 5), panels in HBM, Jacobi, slopes between caps 8 and 32 at tol 0
(a solve's one-time work taken out), --repeats interleaved repeats of everything:

  one rank      k = 8 and 32: fs_dist_pcgn_lambdas with EQUAL lambdas against fs_dist_pcgn in the same run.  The bar: within 3 % (the
                2.4 % the per-column diagonal costs on one device, profiles/pcgn_lambdas_compare.json, rounded up) plus fs_dist_pcgn's
                own spread over its repeats.  The ratio is recorded; outside the bar the JSON says so.
  three ranks   virtual ranks on the one device: host-issue-bound by construction, NOT a scaling result.  k = 8 and 32, the ladder of
                lambdas, scheme 0 against scheme 1.  On one GPU the replicated vector work runs three times over, so scheme 1 must not
                be slower than scheme 0 beyond the two spreads; both medians and the difference are recorded.
  ladder        the column-scaled recipe of tools/pcg_compare.py (10 M x 1 M, 8 per row) on three virtual ranks: the 8 rungs in ONE
                fs_dist_pcgn_lambdas against eight fs_dist_pcg Jacobi solves, in both schemes; recorded without a bar.

Nothing here is a result for more than one real GPU.

    python tools/dist_pcgn_lambdas_compare.py --out profiles/dist_pcgn_lambdas_compare.json"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from dist_pcg_compare import LAM, N, Sharded, capped_slope, panels, wall  # noqa: E402
from libfastsparse_amd import capi  # noqa: E402

LADDER = (1.0, 3.0, 10.0, 30.0, 100.0, 1e3, 1e4, 1e6)
KS = (8, 32)
VIRTUAL = "virtual ranks, not a scaling result: the one process issues every rank's launches, the ranks share one GPU"


def rungs(lam, k):
    return [lam * LADDER[j % 8] * (1.0 + 0.25 * (j // 8)) for j in range(k)]


def stats(v):
    v = sorted(v)
    return {"ms_per_iteration": [round(p, 4) for p in v], "median": round(v[len(v) // 2], 4), "spread": round(v[-1] - v[0], 4)}


def with_scheme(scheme, f):
    capi.set_option("dist_cg_scheme", scheme)
    try:
        return f()
    finally:
        capi.set_option("dist_cg_scheme", 0)


LAST_COUNTS = {}


def capped(infos, cap, every=True):
    """the info of the longest column of a solve at tol 0.  every: all columns have to run to the cap (equal lambdas do; on the ladder
    a column at a huge lambda may reach a residual of exactly 0 and freeze: the counts are recorded)"""
    LAST_COUNTS[cap] = [i.iterations for i in infos]
    assert not every or all(i.iterations == cap and i.converged == 0 for i in infos), [(i.iterations, i.converged) for i in infos]
    return max(infos, key=lambda i: i.iterations)


def one_rank(args, out):
    S = Sharded(args.n, 1)
    b = torch.sin(19.0 * torch.arange(args.n, device="cuda", dtype=torch.float64) + 0.4)
    rec = {"system": f"config 2 pattern, {args.n} x {args.n}, 16 per row, lambda {LAM}; one rank; Jacobi; slopes between caps 8 and 32 at tol 0"}
    for k in KS:
        X, B = panels(b, k)
        solves = {
            "fs_dist_pcgn": lambda c: capped(capi.dist_pcgn(S.M, X, B, LAM, 0.0, max_iter=c, precond=capi.FS_PRECOND_JACOBI), c),
            "fs_dist_pcgn_lambdas_equal": lambda c: capped(capi.dist_pcgn_lambdas(S.M, X, B, [LAM] * k, 0.0, max_iter=c,
                                                                                  precond=capi.FS_PRECOND_JACOBI), c),
        }
        for f in solves.values():
            f(3)
        per = {name: [] for name in solves}
        for _ in range(args.repeats):                                # interleaved, so that drift meets both alike
            for name, f in solves.items():
                per[name].append(capped_slope(f)[0])
        r = {name: stats(v) for name, v in per.items()}
        base = r["fs_dist_pcgn"]
        r["ratio"] = round(r["fs_dist_pcgn_lambdas_equal"]["median"] / base["median"], 4)
        r["bar"] = round(1.03 + base["spread"] / base["median"], 4)
        r["within_bar"] = bool(r["ratio"] <= r["bar"])
        if not r["within_bar"]:
            r["note"] = ("outside 3 % + fs_dist_pcgn's spread: the per-column inverse (one division per element and column in the "
                         "start, update and direction kernels) is what the two solves differ in")
        rec[f"k{k}"] = r
        print("one rank", k, r, flush=True)
    out["one_rank"] = rec
    S.close()


def three_ranks(args, out):
    S = Sharded(args.n, 3)
    b = torch.sin(19.0 * torch.arange(args.n, device="cuda", dtype=torch.float64) + 0.4)
    rec = {"system": f"config 2 pattern, {args.n} x {args.n}, 16 per row, lambda {LAM} x the ladder; three VIRTUAL ranks on one device; Jacobi",
           "note": VIRTUAL}
    for k in KS:
        X, B = panels(b, k)
        lams = rungs(LAM, k)
        def solve(c):
            return capped(capi.dist_pcgn_lambdas(S.M, X, B, lams, 0.0, max_iter=c, precond=capi.FS_PRECOND_JACOBI), c, every=False)
        # the scheme is set once per slope, not per solve: setting an option makes the next k-column solve prepare its shards again,
        # which the untimed first solve of capped_slope then takes
        per = {f"scheme{scheme}": [] for scheme in (0, 1)}
        for _ in range(args.repeats):
            for scheme in (0, 1):
                per[f"scheme{scheme}"].append(with_scheme(scheme, lambda: capped_slope(solve)[0]))
        r = {name: stats(v) for name, v in per.items()}
        r["counts_at_cap_32"] = LAST_COUNTS.get(32)
        r["scheme1_minus_scheme0_ms"] = round(r["scheme1"]["median"] - r["scheme0"]["median"], 4)
        r["scheme1_not_slower_beyond_the_spreads"] = bool(r["scheme1_minus_scheme0_ms"] <= r["scheme0"]["spread"] + r["scheme1"]["spread"])
        rec[f"k{k}"] = r
        print("three ranks", k, r, flush=True)
    out["three_virtual_ranks"] = rec
    S.close()


def ladder(args, out):
    """the column-scaled recipe as three row shards of A, A' built on the devices"""
    L = capi.lib()
    nrow, ncol, per, ranks = args.nrow, args.ncol, 8, 3
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    nnz = nrow * per
    cols = torch.randint(0, ncol, (nnz,), device="cuda", dtype=torch.int32, generator=g)
    scale = 10.0 ** (torch.rand(ncol, device="cuda", dtype=torch.float64, generator=g) * 3.0 - 1.5)
    vals = torch.randn(nnz, device="cuda", dtype=torch.float64, generator=g) * scale[cols.long()]
    lam, tol = 1e-3, 1e-8
    D = L.fs_dist_create(ranks, (C.c_int * ranks)(*([0] * ranks)))
    assert D, L.fs_last_error()
    cuts = [nrow * r // ranks for r in range(ranks + 1)]
    rps = [torch.arange(0, (cuts[r + 1] - cuts[r]) * per + 1, per, device="cuda", dtype=torch.int32) for r in range(ranks)]
    ccs = [cols[cuts[r] * per:cuts[r + 1] * per].contiguous() for r in range(ranks)]
    vvs = [vals[cuts[r] * per:cuts[r + 1] * per].contiguous() for r in range(ranks)]
    M = L.fs_dist_csr_create_from_shards(D, nrow, ncol, (C.c_int * ranks)(*[cuts[r + 1] - cuts[r] for r in range(ranks)]),
                                         (C.c_int64 * ranks)(*[int(c.numel()) for c in ccs]), (C.c_void_p * ranks)(*[t.data_ptr() for t in rps]),
                                         (C.c_void_p * ranks)(*[t.data_ptr() for t in ccs]), (C.c_void_p * ranks)(*[t.data_ptr() for t in vvs]),
                                         capi.FS_DEVICE)
    assert M, L.fs_last_error()
    del rps, ccs, vvs, cols, vals
    capi.check(L.fs_dist_matrix_build_transpose_device(M), "fs_dist_matrix_build_transpose_device")
    b = torch.randn(ncol, device="cuda", dtype=torch.float64, generator=g)
    lams = rungs(lam, 8)
    x = torch.empty(ncol, dtype=torch.float64, device="cuda")
    B = b[:, None].repeat(1, 8).contiguous()
    X = torch.empty_like(B)
    rec = {"system": f"column-scaled, {nrow} x {ncol}, {per} per row, lambda {lam} x the ladder, tol {tol}, cap {args.cap}; three VIRTUAL ranks; Jacobi",
           "note": VIRTUAL, "lambdas": lams}
    def both(scheme):
        capi.dist_pcgn_lambdas(M, X, B, lams, tol, max_iter=3)       # warm: the one-time work of k = 8 under the options as they are now
        infos, ms = wall(lambda: capi.dist_pcgn_lambdas(M, X, B, lams, tol, max_iter=args.cap))
        one = {"ms": round(ms, 3), "counts": [i.iterations for i in infos], "converged": [i.converged for i in infos]}
        capi.dist_pcg(M, x, b, lams[0], tol, max_iter=3)
        each, total = [], 0.0
        for lam_j in lams:
            info, ms = wall(lambda: capi.dist_pcg(M, x, b, lam_j, tol, max_iter=args.cap))
            each.append(info)
            total += ms
        eight = {"ms": round(total, 3), "counts": [i.iterations for i in each], "converged": [i.converged for i in each]}
        return {"one_fs_dist_pcgn_lambdas": one, "eight_fs_dist_pcg_jacobi": eight, "one_solve_over_eight": round(one["ms"] / eight["ms"], 3)}

    for scheme in (0, 1):
        rec[f"scheme{scheme}"] = with_scheme(scheme, lambda: both(scheme))
        print("ladder scheme", scheme, rec[f"scheme{scheme}"], flush=True)
    out["ladder_scaled"] = rec
    L.fs_dist_matrix_destroy(M)
    L.fs_dist_destroy(D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="one,three,ladder")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=N, help="rows and columns of config 2's pattern (a rehearsal at a small size says nothing about speed)")
    ap.add_argument("--nrow", type=int, default=10_000_000)
    ap.add_argument("--ncol", type=int, default=1_000_000)
    ap.add_argument("--cap", type=int, default=1000, help="iteration cap of the solves on the ladder")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0),
           "scope": "one GPU; nothing here is a result for more than one real GPU"}
    what = args.what.split(",")
    for name, f in (("one", one_rank), ("three", three_ranks), ("ladder", ladder)):
        if name in what:
            f(args, out)
            if args.out:                                             # (kept after every part: a later part that fails loses nothing)
                with open(args.out, "w") as fh:
                    json.dump(out, fh, indent=1)
                    fh.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
