"""A pure-Python restatement of the host planners of the copy builders (libfastsparse_amd/csrc/fs_plan.h).

Every function takes and returns plain ints and lists, in the order of operations of the C++ (Python floats are the same
IEEE doubles, int() truncates like a C cast, // is C's division on the non-negative numbers met here), so that the
outputs must agree element for element: tests/test_format_plans.py compares them with tests/plan_driver.cpp on the
CPU, tests/test_gpu_parity.py with what the device builders really laid out.
"""
from bisect import bisect_left, bisect_right

# fs_geometry.h
K_TILED_ITEM, K_TILED_ROWS_MAX, K_TILED_COL_BITS = 2048, 13056, 18
K_LDSX_ROWS, K_LDSX_COLS = 14336, 2048
K_BIN_COLS, K_BIN_ROWS_MAX, K_BIN_COLS_BIG, K_BIN_ROWS_BIG, K_BIN_BIG_RUN_ENTRIES, K_BIN_GROUP = 16384, 16384, 19456, 19456, 192, 16
K_LONG_OWNERS = 16
CONSTS = {"kTiledItem": K_TILED_ITEM, "kTiledRowsMax": K_TILED_ROWS_MAX, "kTiledColBits": K_TILED_COL_BITS, "kLdsxRows": K_LDSX_ROWS,
          "kLdsxCols": K_LDSX_COLS, "kBinCols": K_BIN_COLS, "kBinRowsMax": K_BIN_ROWS_MAX, "kBinColsBig": K_BIN_COLS_BIG,
          "kBinRowsBig": K_BIN_ROWS_BIG, "kBinBigRunEntries": K_BIN_BIG_RUN_ENTRIES, "kBinGroup": K_BIN_GROUP,
          "kLongOwners": K_LONG_OWNERS}


def tiled_slots(ncu):
    """workgroups of the tiled kernels resident together: one per CU, a multiple of the 8 XCDs (build_tiled_impl)"""
    return (ncu if ncu > 8 else 256) // 8 * 8


def plan_tiled_rows(nvrow, slots, rows_max, ldsx, tile_rows):
    R = tile_rows
    if R <= 0:
        g = (nvrow + slots * rows_max - 1) // (slots * rows_max)
        R = (nvrow + slots * g - 1) // (slots * g)
        if R < 256:
            R = nvrow if nvrow < 256 else 256
        if ldsx and nvrow < slots * rows_max // 2:
            np_ = (nvrow + rows_max - 1) // rows_max
            R = (nvrow + np_ - 1) // (np_ if np_ > 0 else 1)
    return min(R, rows_max)


def plan_tiled_panels(nvrow, R, virt, vp, nnz, split):
    panel_row = []
    if not virt:
        panel_row = list(range(0, nvrow, R))
    else:
        cap = int(0.8 * float(nnz) * R / nvrow) + split
        r = 0
        while r < nvrow:
            panel_row.append(r)
            e = r + R if r + R < nvrow else nvrow
            if vp[e] - vp[r] > cap:
                e = bisect_right(vp, vp[r] + cap, r + 1, e + 1) - 1
                if e <= r:
                    e = r + 1
            r = e
    return panel_row + [nvrow]


def plan_band_width(ncol, nnz, P, ldsx, tile_cols):
    w_max = K_LDSX_COLS if ldsx else 1 << K_TILED_COL_BITS
    W = tile_cols
    if W <= 0:
        w = (0.95 if ldsx else 0.9) * K_TILED_ITEM * float(ncol) * P / float(nnz)
        lo = 256 if ldsx else 4096
        if w < lo:
            w = lo
        if w > w_max:
            w = w_max
        W = int(w)
    W = min(W, w_max, ncol)
    if ldsx and (W & 1) and W < w_max:
        W += 1
    return W, (ncol + W - 1) // W


def cut_work_items(tp, P, J):
    items, item_ptr = [], []
    for p in range(P):
        item_ptr.append(len(items))
        for j in range(J):
            a, b = tp[p * J + j], tp[p * J + j + 1]
            for off in range(a, b, K_TILED_ITEM):
                items.append((off, min(b - off, K_TILED_ITEM), j, 0))
    return items, item_ptr + [len(items)]


def count_work_items(tp):
    """what cut_work_items would make, without making them"""
    return sum(-(-(b - a) // K_TILED_ITEM) for a, b in zip(tp[:-1], tp[1:]))


def plan_ldsx_chunks(item_ptr, nitems, P, slots, plain_order):
    total = P if P >= slots else 8 * slots
    n_p = [item_ptr[p + 1] - item_ptr[p] for p in range(P)]
    k_p, frac, given = [], [], 0
    for p in range(P):
        share = float(n_p[p]) * float(total) / float(nitems if nitems else 1)
        cap = n_p[p] if n_p[p] > 0 else 1
        k = min(max(int(share), 1), cap)
        k_p.append(k)
        given += k
        if k < cap:
            frac.append((share - float(int(share)), p))
    frac.sort(key=lambda f: (-f[0], f[1]))
    for _, p in frac:
        if given >= total:
            break
        k_p[p] += 1
        given += 1
    chunks, shared = [], False
    for p in range(P):
        i, i1, k, done = item_ptr[p], item_ptr[p + 1], k_p[p], 0
        shared = shared or k > 1
        for c in range(k):
            first, goal = i, n_p[p] * (c + 1) // k
            while i < i1 and (done < goal or c == k - 1):
                i += 1
                done += 1
            chunks.append((p - (1 << 31) if k > 1 else p, first, i, c))
    if shared:
        if plain_order:
            chunks.sort(key=lambda c: c[3])
        else:
            chunks.sort(key=lambda c: (c[3] >> 3, c[0] & 0x7fffffff, c[3] & 7))
    return {"shared": [int(shared)], "chunk_panel": [c[0] for c in chunks], "chunk_item": [v for c in chunks for v in c[1:3]],
            "chunk_ord": [c[3] for c in chunks]}


def plan_two_pass_geometry(nrow, ncol, nnz, kw, bin_rows, big_env):
    per_run = float(nnz) / (float((ncol + K_BIN_COLS - 1) // K_BIN_COLS) * float((nrow + K_BIN_ROWS_MAX - 1) // K_BIN_ROWS_MAX))
    big = kw == 1 and bin_rows == 0 and (big_env != 0 if big_env >= 0 else per_run < K_BIN_BIG_RUN_ENTRIES)
    bcols = K_BIN_COLS_BIG if big else K_BIN_COLS // kw
    rmax = K_BIN_ROWS_BIG if big else K_BIN_ROWS_MAX // kw
    R = min(bin_rows if bin_rows > 0 else rmax, rmax)
    return {"big": int(big), "bcols": bcols, "rmax": rmax, "ge": K_BIN_GROUP // kw, "R": R}


def plan_two_pass_panels(vp, nvrow, nnz, R, slots, fill, min_panels, kw):
    want = int(float(nvrow) / (fill * R)) + 1
    if want > slots:
        want = (want + slots - 1) // slots * slots
    if min_panels and want < slots and nvrow >= slots * 256 and kw == 1:
        want = slots
    panel_row, r, k = [], 0, 1
    while k <= want and r < nvrow:
        goal = int(float(nnz) * float(k) / float(want))
        e = bisect_left(vp, goal, r, len(vp))
        if e > r and e <= nvrow and vp[e] - goal > goal - vp[e - 1] and e - 1 > r:
            e -= 1
        if k == want or e > nvrow:
            e = nvrow
        while r < e:
            panel_row.append(r)
            r = r + R if e - r > R else e
        k += 1
    if not panel_row:
        panel_row.append(0)
    return panel_row + [nvrow]


def deal_long_rows(cands, cap_rows):
    """cands: (row, entries) pairs in any order"""
    h = sorted(cands, key=lambda c: (-c[1], c[0]))[:cap_rows]
    blk = [[] for _ in range(K_LONG_OWNERS)]
    for i, c in enumerate(h):
        lap, pos = divmod(i, K_LONG_OWNERS)
        blk[K_LONG_OWNERS - 1 - pos if lap & 1 else pos].append(c)
    h, own_first = [], []
    for b in blk:
        own_first.append(len(h))
        h += sorted(b, key=lambda c: c[0])
    own_first.append(len(h))
    owner_of = [w for w in range(K_LONG_OWNERS) for _ in range(own_first[w], own_first[w + 1])]
    lptr = [0]
    for _, n in h:
        lptr.append(lptr[-1] + n)
    return {"rows": [c[0] for c in h], "own_first": own_first, "owner_of": owner_of, "lptr": lptr}


def pad_long_segments(hs, B):
    hp, hseg, hsh, at = [0] * (B + 1), [0] * (B * (K_LONG_OWNERS + 1)), [0] * (B * K_LONG_OWNERS + 1), 0
    for b in range(B):
        hp[b] = at
        for w in range(K_LONG_OWNERS):
            sg = b * K_LONG_OWNERS + w
            hseg[b * (K_LONG_OWNERS + 1) + w] = (at - hp[b]) & 0xffffffff
            hsh[sg] = at - hs[sg]
            at += (hs[sg + 1] - hs[sg] + 1) & ~1
        hseg[b * (K_LONG_OWNERS + 1) + K_LONG_OWNERS] = (at - hp[b]) & 0xffffffff
        if at - hp[b] >= 1 << 32:
            return {"ok": [0], "hp": hp, "hseg": hseg, "hsh": hsh}
    hp[B] = at
    return {"ok": [1], "hp": hp, "hseg": hseg, "hsh": hsh}


def plan_generation_cuts(nunits, slots, nparts):
    """units[0 .. nparts] of a launch of nunits workgroups in parts: whole generations of `slots` resident workgroups"""
    gens = (nunits + slots - 1) // slots
    c = min(nparts, gens)
    return [min(nunits, slots * (gens * p // c)) if p < c else nunits for p in range(nparts + 1)]


# ---- what the device steps around the planners do, for predictions from a CSR (numpy) -------------------------------------
def virtual_rows(rp, split):
    """entry offsets of the virtual rows (nvrow + 1): rows longer than `split` cut into pieces of `split` consecutive entries
    (piece_count_kernel / vrow_fill_kernel); the rows themselves when none is longer"""
    import numpy as np
    rp = np.asarray(rp, dtype=np.int64)
    lens = np.diff(rp)
    if lens.size == 0 or lens.max() <= split:
        return [int(v) for v in rp], False
    pieces = np.where(lens <= split, 1, -(-lens // split))
    first = np.concatenate(([0], np.cumsum(pieces)))
    vp = np.repeat(rp[:-1], pieces) + (np.arange(first[-1]) - np.repeat(first[:-1], pieces)) * split
    return [int(v) for v in vp] + [int(rp[-1])], True


def tile_pointers(vp, panel_row, cols, W, J):
    """tile_ptr of the (panel, band) tiles (P * J + 1): what the sort by tile_key_kernel's keys and tile_ptr_kernel give"""
    import numpy as np
    nnz, P = len(cols), len(panel_row) - 1
    v = np.searchsorted(np.asarray(vp[:-1]), np.arange(nnz), side="right") - 1          # last virtual row that starts at or before the entry
    p = np.searchsorted(np.asarray(panel_row[:-1]), v, side="right") - 1
    counts = np.bincount(p * J + np.asarray(cols, dtype=np.int64) // W, minlength=P * J)
    return [0] + [int(c) for c in np.cumsum(counts)]
