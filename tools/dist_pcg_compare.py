#!/usr/bin/env python3
"""fs_dist_pcg against fs_dist_cg and fs_pcg, one process, one GPU, one JSON file.

On config 2's pattern (10 M x 10 M, 16 per row, pattern-only, lambda 5), vectors in HBM, --repeats interleaved repeats of everything:

  one rank      fs_dist_cg (it takes no cap: the slope between its solves at tol 1e-3 and 1e-8, as mscg_compare.py does),
                fs_dist_pcg without a preconditioner and with Jacobi (tol 0, the slope between caps 8 and 32: a solve's one-time work
                -- the copies of b and x, the diagonal and its gather, the start -- taken out), and fs_pcg on single-device handles of
                the same pattern, both ways, in the same run.  Two comparisons:
                  fs_dist_pcg without a preconditioner launches fs_dist_cg's kernels: its median has to lie inside the spread of
                  fs_dist_cg's own repeats;
                  Jacobi's surcharge per iteration on the sharded path against 1.5 x the surcharge fs_pcg shows in this run.
  three ranks   virtual ranks on the one device: host-issue-bound by construction, NOT a scaling result.  Scheme 0 against scheme 1,
                without a preconditioner and with Jacobi; recorded without a bar.

Both also record the other two sharded solvers, without a bar: fs_dist_cg2 (the slope between tol 1e-3 and 1e-8, like fs_dist_cg)
and fs_dist_pcgn with Jacobi at k = 4 (the slope between caps 8 and 32) -- all four are in one record when two builds are
compared (FS_LIB_PATH names the other build's library).

    python tools/dist_pcg_compare.py --out profiles/dist_pcg_compare.json"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from libfastsparse_amd import capi  # noqa: E402

N, PER_ROW, SEED, LAM = 10_000_000, 16, 0x5EED0002, 5.0


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
        self.ranks = ranks
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


def dist_cg(S, x, b, tol, two=False):
    """fs_dist_cg, or (two: x, b of n x 2) fs_dist_cg2"""
    it = C.c_int(0)
    f = capi.lib().fs_dist_cg2 if two else capi.lib().fs_dist_cg
    _, ms = wall(lambda: capi.check(f(S.M, x.data_ptr(), b.data_ptr(), LAM, tol, C.byref(it)), "fs_dist_cg2" if two else "fs_dist_cg"))
    return it.value + 1, ms


def dist_cg_slope(S, x, b, tols=(1e-3, 1e-8), two=False):
    if two:                                                          # (the handle's k-column work space is fs_dist_pcgn's k = 4 by now:
        dist_cg(S, x, b, tols[0], two)                               #  the switch back to k = 2 is one-time work, outside the timed pair)
    (n1, t1), (n2, t2) = (dist_cg(S, x, b, tol, two) for tol in tols)
    assert n2 > n1, (n1, n2)
    return (t2 - t1) / (n2 - n1), [n1 - 1, n2 - 1]


def panels(b, k):
    """k right-hand sides, n x k row-major: b, then columns no two of which are parallel; and the X of the same shape"""
    i = torch.arange(b.numel(), device="cuda", dtype=torch.float64)
    B = torch.stack([b] + [torch.cos((7.0 + 3.0 * j) * i + 0.1 * j) for j in range(1, k)], 1).contiguous()
    return torch.empty_like(B), B


def dist_pcgn(S, X, B, cap):
    """fs_dist_pcgn with Jacobi at tol 0: every column runs to the cap; the info of column 0"""
    infos = capi.dist_pcgn(S.M, X, B, LAM, 0.0, max_iter=cap, precond=capi.FS_PRECOND_JACOBI)
    assert all(i.iterations == cap and i.converged == 0 for i in infos), [(i.iterations, i.converged) for i in infos]
    return infos[0]


def capped_slope(solve, lo=8, hi=32):
    """ms per iteration between two solves at tol 0 that run exactly lo and hi iterations, and what is left of the shorter one.
    One untimed iteration first: a solve that follows one of another k switches the handle's k-column work space, once"""
    solve(1)
    t = {}
    for n in (lo, hi):
        info, t[n] = wall(lambda: solve(n))
        assert info.iterations == n and info.converged == 0, (n, info.iterations, info.converged)
    per = (t[hi] - t[lo]) / (hi - lo)
    return per, t[lo] - lo * per


def stats(v):
    v = sorted(v)
    return {"ms_per_iteration": [round(p, 4) for p in v], "median": round(v[len(v) // 2], 4)}


def one_rank(args, out):
    n = args.n
    rp, cc, _ = capi.synth_uniform(n, n, PER_ROW, SEED, valued=False)
    A = capi.Matrix.from_csr(n, n, rp, cc, None, borrow=True)
    rows = torch.arange(n, device="cuda", dtype=torch.int32).repeat_interleave(PER_ROW)
    At = capi.Matrix.from_coo(n, n, cc, rows, None)
    del rows
    S = Sharded(n, 1)
    b = torch.sin(19.0 * torch.arange(n, device="cuda", dtype=torch.float64) + 0.4)
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    st = capi.current_stream()
    solves = {
        "fs_pcg_none": lambda c: capi.pcg(A, At, x, b, LAM, 0.0, max_iter=c, precond=capi.FS_PRECOND_NONE, stream=st),
        "fs_pcg_jacobi": lambda c: capi.pcg(A, At, x, b, LAM, 0.0, max_iter=c, precond=capi.FS_PRECOND_JACOBI, stream=st),
        "fs_dist_pcg_none": lambda c: capi.dist_pcg(S.M, x, b, LAM, 0.0, max_iter=c, precond=capi.FS_PRECOND_NONE),
        "fs_dist_pcg_jacobi": lambda c: capi.dist_pcg(S.M, x, b, LAM, 0.0, max_iter=c, precond=capi.FS_PRECOND_JACOBI),
    }
    X2, B2 = panels(b, 2)
    X4, B4 = panels(b, 4)
    solves["fs_dist_pcgn_k4_jacobi"] = lambda c: dist_pcgn(S, X4, B4, c)
    dist_cg(S, x, b, 1e-3)                                           # warm: every kernel, every work space
    dist_cg(S, X2, B2, 1e-3, two=True)
    for f in solves.values():
        f(3)
    per = {k: [] for k in ["fs_dist_cg", "fs_dist_cg2"] + list(solves)}
    once = {k: [] for k in solves}
    counts = counts2 = None
    for _ in range(args.repeats):                                    # interleaved, so that drift meets all of them alike
        p, counts = dist_cg_slope(S, x, b)
        per["fs_dist_cg"].append(p)
        p, counts2 = dist_cg_slope(S, X2, B2, two=True)
        per["fs_dist_cg2"].append(p)
        for k, f in solves.items():
            p, o = capped_slope(f)
            per[k].append(p)
            once[k].append(o)
    rec = {"system": f"config 2 pattern, {n} x {n}, {PER_ROW} per row, lambda {LAM}; one rank; slopes between caps 8 and 32 at tol 0",
           "kernels": {"fs_pcg": [A.kernel_name(), At.kernel_name()]}, "fs_dist_cg_counts_at_tol_1e-3_1e-8": counts,
           "fs_dist_cg2_counts_at_tol_1e-3_1e-8": counts2}
    for k, v in per.items():
        rec[k] = stats(v)
        if k in once:
            rec[k]["one_time_ms"] = [round(o, 3) for o in sorted(once[k])]
        print(k, rec[k], flush=True)
    lo, hi = rec["fs_dist_cg"]["ms_per_iteration"][0], rec["fs_dist_cg"]["ms_per_iteration"][-1]
    rec["fs_dist_cg_spread_ms"] = round(hi - lo, 4)
    rec["none_inside_fs_dist_cg_spread"] = bool(lo <= rec["fs_dist_pcg_none"]["median"] <= hi)
    rec["jacobi_surcharge_fs_pcg_ms"] = round(rec["fs_pcg_jacobi"]["median"] - rec["fs_pcg_none"]["median"], 4)
    rec["jacobi_surcharge_fs_dist_pcg_ms"] = round(rec["fs_dist_pcg_jacobi"]["median"] - rec["fs_dist_pcg_none"]["median"], 4)
    rec["jacobi_surcharge_within_1.5x"] = bool(rec["jacobi_surcharge_fs_dist_pcg_ms"] <= 1.5 * rec["jacobi_surcharge_fs_pcg_ms"])
    out["one_rank"] = rec
    S.close()


def three_ranks(args, out):
    n = args.n
    S = Sharded(n, 3)
    b = torch.sin(19.0 * torch.arange(n, device="cuda", dtype=torch.float64) + 0.4)
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    solves = {}
    for scheme in (0, 1):
        for name, precond in (("none", capi.FS_PRECOND_NONE), ("jacobi", capi.FS_PRECOND_JACOBI)):
            def f(c, scheme=scheme, precond=precond):
                capi.set_option("dist_cg_scheme", scheme)
                try:
                    return capi.dist_pcg(S.M, x, b, LAM, 0.0, max_iter=c, precond=precond)
                finally:
                    capi.set_option("dist_cg_scheme", 0)
            solves[f"scheme{scheme}_{name}"] = f
    X2, B2 = panels(b, 2)
    X4, B4 = panels(b, 4)
    solves["fs_dist_pcgn_k4_jacobi"] = lambda c: dist_pcgn(S, X4, B4, c)         # (replicated whatever the scheme)
    dist_cg(S, x, b, 1e-3)
    dist_cg(S, X2, B2, 1e-3, two=True)
    for f in solves.values():
        f(3)
    per = {k: [] for k in ["fs_dist_cg", "fs_dist_cg2"] + list(solves)}
    for _ in range(args.repeats):
        per["fs_dist_cg"].append(dist_cg_slope(S, x, b)[0])
        per["fs_dist_cg2"].append(dist_cg_slope(S, X2, B2, two=True)[0])
        for k, f in solves.items():
            per[k].append(capped_slope(f)[0])
    rec = {"system": f"config 2 pattern, {n} x {n}, {PER_ROW} per row, lambda {LAM}; three VIRTUAL ranks on one device",
           "note": "virtual ranks, not a scaling result: the one process issues every rank's launches, the ranks share one GPU"}
    for k, v in per.items():
        rec[k] = stats(v)
        print(k, rec[k], flush=True)
    out["three_virtual_ranks"] = rec
    S.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="one,three")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=N, help="rows and columns (a rehearsal at a small size says nothing about speed)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    if "one" in args.what.split(","):
        one_rank(args, out)
    if "three" in args.what.split(","):
        three_ranks(args, out)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
