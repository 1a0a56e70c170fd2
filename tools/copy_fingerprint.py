"""Fingerprint of what the copy builders lay out (csrc/fs_copies.hip), for changes that must not move one entry.

  python tools/copy_fingerprint.py --out FILE.json [--small]     one JSON record per matrix and forced path, with the
                                                                 library that FS_LIB_PATH names (default: the product build)
  python tools/copy_fingerprint.py --compare A.json B.json       field-for-field comparison; exit status 1 when they differ

Run the two libraries in fresh processes of their own.  A record holds the kernel kept, fs_matrix_device_bytes, the geometry
and layout the fs_debug_* readers report, the plans of k = 2 and 4 column products, and SHA-256 digests of y = A x, z = A' u and
of fs_spmm for k = 2, 4 under reproducible = 1 (set after creation): with fixed-order sums the bits of a product are a function
of the stored order of the entries, so they fingerprint the layout.  Digests are recorded only where
fs_debug_fixed_order_honoured says the order is fixed.
Matrices: syn_u16_2048, syn_long_800x5000 (cut rows), syn_wide_300x40000 of tests/_cases.py; unless --small, synth_uniform
1 M x 1 M x 16 (above the auto thresholds of every path) and the same with one row of 200 000 entries (long rows are taken).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEFAULTS = {"tiling": 1, "ldsx": 1, "binning": 1, "bin_flags": 0, "long_rows": 1, "long_min_len": 0, "tile_split": 0, "reproducible": 0}
PATHS = [("stream", {"tiling": 0, "ldsx": 0, "binning": 0}),
         ("two-pass 64", {"binning": 2, "bin_flags": 64}),
         ("two-pass 128", {"binning": 2, "bin_flags": 128}),
         ("long rows", {"binning": 2, "long_rows": 2, "long_min_len": 32}),
         ("lds-staged", {"ldsx": 2}),
         ("tiled cut rows", {"tiling": 2, "tile_split": 5})]


def compare(a, b):
    ra, rb = json.load(open(a)), json.load(open(b))
    bad = 0
    if [r["id"] for r in ra] != [r["id"] for r in rb]:
        print("different records:", [r["id"] for r in ra], [r["id"] for r in rb])
        return 1
    for x, y in zip(ra, rb):
        for k in sorted(set(x) | set(y)):
            if x.get(k) != y.get(k):
                print("%s: %s differs: %r | %r" % (x["id"], k, x.get(k), y.get(k)))
                bad += 1
    print("%d records, %d fields differ" % (len(ra), bad))
    return 1 if bad else 0


def matrices(small):
    import torch
    import _cases
    from libfastsparse_amd import capi
    from oracle import pyoracle as O
    for c in _cases.all_cases():
        if c.name in ("syn_u16_2048", "syn_long_800x5000", "syn_wide_300x40000"):
            rp, cc, vv = O.coo_to_csr(c.nrow, c.rows, c.cols, c.vals)
            yield c.name, c.nrow, c.ncol, torch.from_numpy(rp).cuda(), torch.from_numpy(cc).cuda(), torch.from_numpy(vv).cuda()
    if small:
        return
    n = 1_000_000
    yield ("uniform_1Mx1Mx16", n, n) + capi.synth_uniform(n, n, 16, 0x5EED11)
    lens = torch.full((n,), 16, dtype=torch.int64, device="cuda")
    lens[123_456] = 200_000
    rp = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lens, 0, out=rp[1:])
    rp = rp.to(torch.int32)
    nnz = int(rp[-1].item())
    cc = torch.empty(nnz, dtype=torch.int32, device="cuda")
    vv = torch.empty(nnz, dtype=torch.float64, device="cuda")
    capi.check(capi.lib().fs_synth_fill(n, n, 0x5EED12, 0, capi._ptr(rp), capi._ptr(cc), capi._ptr(vv), capi.current_stream()))
    yield "uniform_1Mx1Mx16_one_row_200000", n, n, rp, cc, vv


def fingerprint(out, small):
    import torch
    import _synth as S
    from libfastsparse_amd import capi
    L = capi.lib()
    L.fs_debug_tiled_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.fs_debug_two_pass_layout.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]
    L.fs_debug_long_rows.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    L.fs_debug_two_pass_rows8.restype = C.c_longlong
    for f in ("fs_debug_tiled_layout", "fs_debug_ldsx_orderable", "fs_debug_fixed_order_honoured", "fs_debug_two_pass_rows8"):
        getattr(L, f).argtypes = [C.c_void_p, C.c_int]

    def sha(t):
        torch.cuda.synchronize()
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    records = []
    for name, nrow, ncol, rp, cc, vv in matrices(small):
        x = torch.from_numpy(S.x_sin(ncol)).cuda()
        u = torch.from_numpy(S.x_sin(nrow, 11.0, -0.2)).cuda()
        for path, opts in PATHS:
            for k, v in {**DEFAULTS, **opts}.items():
                capi.set_option(k, v)
            A = capi.Matrix.from_csr(nrow, ncol, rp, cc, vv)
            A.build_transpose()
            rec = {"id": "%s / %s" % (name, path)}
            for t in (0, 1):
                s = "_t" if t else ""
                rec["kernel" + s] = A.kernel_name(bool(t))
                geo, lay, lr = (C.c_int * 6)(), (C.c_ulonglong * 8)(), (C.c_int64 * 2)()
                if not t:
                    rec["tiled_geometry"] = list(geo) if L.fs_debug_tiled_geometry(A.h, geo) == 0 else None
                rec["tiled_layout" + s] = L.fs_debug_tiled_layout(A.h, t)
                rec["ldsx_orderable" + s] = L.fs_debug_ldsx_orderable(A.h, t)
                rec["two_pass_nBP" + s] = [int(v) for v in lay[5:8]] if L.fs_debug_two_pass_layout(A.h, t, lay) == 0 else None
                rec["two_pass_rows8" + s] = int(L.fs_debug_two_pass_rows8(A.h, t))
                rec["long_rows" + s] = [int(v) for v in lr] if L.fs_debug_long_rows(A.h, t, lr) == 0 else None
            rec["device_bytes"] = [int(v) for v in A.device_bytes()]
            capi.set_option("reproducible", 1)                       # after creation: the copies stay as they were built
            for t, vec, n_out in ((0, x, nrow), (1, u, ncol)):
                y = torch.full((n_out,), -1.0, dtype=torch.float64, device="cuda")
                A.spmv(y, vec, capi.current_stream(), transposed=bool(t))
                honoured = L.fs_debug_fixed_order_honoured(A.h, t)
                rec["fixed_order_honoured" + ("_t" if t else "")] = honoured
                rec["sha256_" + ("z" if t else "y")] = sha(y) if honoured == 1 else None
            for k in (2, 4):
                A.prepare(k, capi.current_stream())
                rec["spmm_plan_k%d" % k] = A.spmm_plan(k)
                X = torch.from_numpy(S.X_sin(ncol, k)).cuda()
                Y = torch.full((nrow, k), -1.0, dtype=torch.float64, device="cuda")
                A.spmm(Y, X, k, capi.current_stream())
                honoured = L.fs_debug_fixed_order_honoured(A.h, 0)     # asked again: the k-column copy was built in between
                rec["fixed_order_honoured_k%d" % k] = honoured
                rec["sha256_spmm_k%d" % k] = sha(Y) if honoured == 1 else None
            rec["device_bytes_prepared"] = [int(v) for v in A.device_bytes()]
            A.close()
            records.append(rec)
            print(json.dumps(rec), flush=True)
    for k, v in DEFAULTS.items():
        capi.set_option(k, v)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="the three small cases only")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    fingerprint(a.out, a.small)
