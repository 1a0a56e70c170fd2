"""The host planners of the copy builders (libfastsparse_amd/csrc/fs_plan.h) on the CPU alone.

tests/plan_driver.cpp -- a stand-alone program around fs_plan.h -- is compiled with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer and run ONCE as a child process on every case below.  Two things are asserted:
  1. its outputs equal tests/_plan_model.py's, element for element;
  2. properties the kernels rely on, stated without the model.
"""
import os
import random
import shutil
import subprocess

import pytest

import _plan_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "libfastsparse_amd", "csrc")
INT_MAX = 2**31 - 1
NVROWS = (1, 255, 256, 257, 5000)
SLOTS = (8, 256)


def _vec(v):
    return "%d %s" % (len(v), " ".join(str(int(x)) for x in v))


def _row_ptr(lens):
    rp = [0]
    for n in lens:
        rp.append(rp[-1] + n)
    return rp


def _lens(rng, nrow, heavy):
    """row lengths 0 .. 9; heavy: one row holds 90 % of the entries"""
    lens = [rng.randrange(0, 10) for _ in range(nrow)]
    if heavy:
        lens[nrow // 3] = 9 * max(sum(lens) - lens[nrow // 3], 1)
    return lens


def _virtual_rows(rp, split):
    """entry offsets of the virtual rows: rows longer than `split` cut into pieces of `split` (piece_count / vrow_fill kernels)"""
    vp = []
    for a, b in zip(rp[:-1], rp[1:]):
        vp += list(range(a, b, split)) if b - a > split else [a]
    return vp + [rp[-1]]


def _cases():
    """(command line for the driver, the model's outputs, what the property checks need)"""
    rng = random.Random(20240607)
    out = [("consts", {"consts": list(M.CONSTS.values())}, {})]
    for nvrow in NVROWS:
        for slots in SLOTS:
            for ldsx in (0, 1):
                rows_max = M.K_LDSX_ROWS if ldsx else M.K_TILED_ROWS_MAX
                for tile_rows in (0, 64):
                    R = M.plan_tiled_rows(nvrow, slots, rows_max, ldsx, tile_rows)
                    out.append(("tiled_rows %d %d %d %d %d" % (nvrow, slots, rows_max, ldsx, tile_rows), {"R": [R]}, {}))
                    # rows as they are ...
                    out.append(("tiled_panels %d %d 0 %d 256 0" % (nvrow, R, 7 * nvrow),
                                {"panel_row": M.plan_tiled_panels(nvrow, R, False, [], 7 * nvrow, 256)}, {"panels": (nvrow, R)}))
                # ... and cut ones, with and without a row that holds 90 % of the entries (L2-tiled copy only)
                for heavy in (False, True):
                    for split in (5, 256):
                        vp = _virtual_rows(_row_ptr(_lens(rng, nvrow, heavy)), split)
                        nv, nnz = len(vp) - 1, vp[-1]
                        if nnz == 0:
                            continue
                        for tile_rows in (0, 64):
                            R = M.plan_tiled_rows(nv, slots, M.K_TILED_ROWS_MAX, 0, tile_rows)
                            out.append(("tiled_panels %d %d 1 %d %d %s" % (nv, R, nnz, split, _vec(vp)),
                                        {"panel_row": M.plan_tiled_panels(nv, R, True, vp, nnz, split)}, {"panels": (nv, R)}))
    for ncol, nnz, P in ((1, 1, 1), (70, 20000, 1), (2048, 32768, 8), (40000, 12000, 1), (5000, 52000, 13), (1000000, 16000000, 1024),
                         (300001, 5000000, 3)):
        for ldsx in (0, 1):
            for tile_cols in (0, 128):
                W, J = M.plan_band_width(ncol, nnz, P, ldsx, tile_cols)
                out.append(("band_width %d %d %d %d %d" % (ncol, nnz, P, ldsx, tile_cols), {"WJ": [W, J]}, {"band": (ncol, ldsx)}))
    # work items: tiles of 0, 1, a whole item, one more, several items
    for P, J in ((1, 1), (3, 4), (7, 1), (2, 9)):
        sizes = [rng.choice((0, 0, 1, 5, 2047, 2048, 2049, 4096, 7000)) for _ in range(P * J)]
        tp = _row_ptr(sizes)
        items, item_ptr = M.cut_work_items(tp, P, J)
        out.append(("work_items %d %d 1 %s" % (P, J, _vec(tp)),
                    {"nitems": [len(items)], "item_ptr": item_ptr, "items": [v for it in items for v in it]}, {"items": (tp, P, J)}))
    tp = [0, INT_MAX - 100]        # entry offsets within 2 047 of INT_MAX: a 32-bit offset wrapped around and the cutter never ended
    out.append(("work_items 1 1 0 %s" % _vec(tp), {"nitems": [M.count_work_items(tp)], "item_ptr": [0, M.count_work_items(tp)]},
                {"int_max": True}))
    # chunks: fewer panels than slots, as many, more; equal panels, unequal ones, a panel without items
    for slots in SLOTS:
        for P in (1, 3, slots - 1, slots, slots + 1, 3 * slots + 5):
            for kind in ("equal", "unequal", "empty panel", "few items"):
                if kind == "equal":
                    n_p = [40] * P
                elif kind == "few items":
                    n_p = [rng.randrange(0, 3) for _ in range(P)]
                else:
                    n_p = [rng.randrange(1, 400) for _ in range(P)]
                    if kind == "empty panel":
                        n_p[P // 2] = 0
                item_ptr = _row_ptr(n_p)
                for plain in (0, 1):
                    out.append(("ldsx_chunks %d %d %d %d %s" % (P, slots, plain, item_ptr[-1], _vec(item_ptr)),
                                M.plan_ldsx_chunks(item_ptr, item_ptr[-1], P, slots, plain), {"chunks": (item_ptr, P, slots, plain)}))
    for kw in (1, 2, 4):
        for bin_rows in (0, 64):
            for big_env in (-1, 0, 1):
                for nrow, ncol, nnz in ((300, 40000, 12000), (10**7, 10**7, 16 * 10**7), (2 * 10**6, 5 * 10**7, 10**7)):
                    g = M.plan_two_pass_geometry(nrow, ncol, nnz, kw, bin_rows, big_env)
                    out.append(("two_pass_geometry %d %d %d %d %d %d" % (nrow, ncol, nnz, kw, bin_rows, big_env),
                                {"geometry": [g["big"], g["bcols"], g["rmax"], g["ge"], g["R"]]}, {}))
    for slots in SLOTS:
        for nrow in NVROWS + (slots * 256 - 1, slots * 256):
            for heavy in (False, True):
                vp = _virtual_rows(_row_ptr(_lens(rng, nrow, heavy)), 256)
                nv, nnz = len(vp) - 1, vp[-1]
                big = nrow >= slots * 256 - 1        # (the min_panels threshold, kw = 1 only: the long inputs are not run for every kw)
                for kw in (1, 2, 4):
                    for bin_rows in (0, 64):
                        for min_panels in (0, 1):
                            if big and nrow > 5000 and (kw, bin_rows) not in ((1, 0), (2, 0)):
                                continue
                            R = M.plan_two_pass_geometry(nrow, 40000, nnz, kw, bin_rows, 0)["R"]
                            out.append(("two_pass_panels %d %d %d %d %r %d %d %s" % (nv, nnz, R, slots, 0.8, min_panels, kw, _vec(vp)),
                                        {"panel_row": M.plan_two_pass_panels(vp, nv, nnz, R, slots, 0.8, min_panels, kw)},
                                        {"panels": (nv, R)}))
    cap_rows = 40
    for ncand in (0, 1, 15, 16, 17, 33, cap_rows + 5):
        rows = rng.sample(range(100000), ncand)
        cands = [(r, rng.choice((600, 600, 600, 777, 5000))) for r in rows]            # tied lengths
        out.append(("long_rows %d %s" % (cap_rows, _vec([v for c in cands for v in c])), M.deal_long_rows(cands, cap_rows),
                    {"long": (cands, cap_rows)}))
    for B, kind in ((1, "mixed"), (3, "mixed"), (4, "empty band"), (2, "odd"), (2, "even")):
        counts = []
        for b in range(B):
            for w in range(M.K_LONG_OWNERS):
                c = rng.randrange(0, 50)
                c = c | 1 if kind == "odd" else c & ~1 if kind == "even" else c
                counts.append(0 if kind == "empty band" and b == 1 else c)
        hs = _row_ptr(counts)
        out.append(("pad_segments %d %s" % (B, _vec(hs)), M.pad_long_segments(hs, B), {"segments": (hs, B)}))
    for nunits, slots, nparts in GENERATION_CUTS:
        out.append(("generation_cuts %d %d %d" % (nunits, slots, nparts), {"units": M.plan_generation_cuts(nunits, slots, nparts)},
                    {"cuts": (nunits, slots, nparts)}))
    return out


# (workgroups, resident together, parts) -> the cuts written out where they are short: config 2's 768 panels in 4 parts take its 3
# generations; config 3's 698 = 256 + 256 + 186 in eight ranges; one workgroup more than a generation; exactly one generation; fewer
# workgroups than slots; many small generations; a count at the int32 limit (64-bit intermediates)
GENERATION_CUTS = {(768, 256, 4): [0, 256, 512, 768, 768], (698, 256, 8): [0, 256, 512] + [698] * 6, (257, 256, 2): [0, 256, 257],
                   (256, 256, 2): None, (1, 8, 7): None, (5000, 8, 7): None, (2**31 - 2, 256, 64): None}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case through the sanitized driver, in one child process"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/plan_driver.cpp")
    cases = _cases()
    exe = str(tmp_path_factory.mktemp("plan") / "plan_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(HERE, "plan_driver.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], input="\n".join(c[0] for c in cases) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got = []
    for line in run.stdout.splitlines():
        key, *vals = line.split()
        if key == "case":
            got.append({})
        else:
            got[-1][key] = [int(v) for v in vals]
    assert len(got) == len(cases)
    return [(cmd, want, meta, g) for (cmd, want, meta), g in zip(cases, got)]


def _with(results, key):
    sel = [(cmd, meta[key], g) for cmd, _, meta, g in results if key in meta]
    assert sel
    return sel


def test_every_planner_equals_its_model(results):
    kinds = set()
    for cmd, want, _, got in results:
        kinds.add(cmd.split()[0])
        assert got == want, cmd[:200]
    assert kinds == {"consts", "tiled_rows", "tiled_panels", "band_width", "work_items", "ldsx_chunks", "two_pass_geometry", "two_pass_panels",
                     "long_rows", "pad_segments", "generation_cuts"}


def test_panels_partition_the_rows(results):
    """first rows of the panels: strictly increasing from 0 to nvrow, at most R rows each (tiled, LDS-staged and two-pass)"""
    for cmd, (nvrow, R), got in _with(results, "panels"):
        pr = got["panel_row"]
        assert pr[0] == 0 and pr[-1] == nvrow, cmd[:120]
        assert all(0 < b - a <= R for a, b in zip(pr[:-1], pr[1:])), cmd[:120]


def test_band_width_fits_the_kernel(results):
    for cmd, (ncol, ldsx), got in _with(results, "band"):
        W, J = got["WJ"]
        assert 1 <= W <= (M.K_LDSX_COLS if ldsx else 1 << M.K_TILED_COL_BITS) and (J - 1) * W < ncol <= J * W, cmd


def test_work_items_cover_every_tile_once_in_order(results):
    for cmd, (tp, P, J), got in _with(results, "items"):
        flat = got["items"]
        items = [tuple(flat[i:i + 4]) for i in range(0, len(flat), 4)]
        assert got["nitems"] == [len(items)] and got["item_ptr"][0] == 0 and got["item_ptr"][-1] == len(items)
        at = 0
        for p in range(P):
            assert got["item_ptr"][p] == at
            for j in range(J):
                pos = tp[p * J + j]
                while pos < tp[p * J + j + 1]:
                    first, count, band, pad = items[at]
                    assert first == pos and 1 <= count <= M.K_TILED_ITEM and band == j and pad == 0, cmd[:120]
                    pos += count
                    at += 1
                assert pos == tp[p * J + j + 1]
        assert at == len(items)


def test_work_items_at_the_int32_limit(results):
    """an entry offset that wrapped near INT_MAX made the cutter loop for ever (270 GB of work items): here in milliseconds"""
    (cmd, _, got), = _with(results, "int_max")
    assert got["nitems"] == [-(-(INT_MAX - 100) // 2048)] and got["item_ptr"] == [0, got["nitems"][0]]


def test_chunks_tile_their_panels_and_launch_in_order(results):
    """A panel's chunks tile its item range contiguously in ordinal order; the shared flag is set iff the panel has more than
    one chunk; the launch order is a permutation of the chunks, sorted by (ordinal >> 3, panel, ordinal & 7) when chunks share
    panels (plain order: by ordinal, panels ascending inside one).

    The chunk count: the builder aims at `total` chunks (P when P >= slots, else 8 per slot).  A panel never gets fewer than
    one, so the count is max(total, sum over the panels of max(floor(share), 1)) with share = the panel's items * total /
    nitems, whenever nitems >= total -- which IS `total` whenever no panel is owed less than one chunk.  (Stated for every
    panel mix it does not hold: items 0, 0, 0, 192 on 8 slots give 1 + 1 + 1 + 64 = 67 chunks, not 64.)"""
    exact = 0
    for cmd, (item_ptr, P, slots, plain), got in _with(results, "chunks"):
        n = len(got["chunk_ord"])
        assert len(got["chunk_panel"]) == n and len(got["chunk_item"]) == 2 * n
        chunks = [(got["chunk_panel"][i] & 0x7fffffff, got["chunk_panel"][i] < 0, got["chunk_item"][2 * i], got["chunk_item"][2 * i + 1],
                   got["chunk_ord"][i]) for i in range(n)]
        per_panel = [sorted((c for c in chunks if c[0] == p), key=lambda c: c[4]) for p in range(P)]
        assert sum(len(q) for q in per_panel) == n                       # no chunk of a panel that does not exist
        for p, q in enumerate(per_panel):
            assert [c[4] for c in q] == list(range(len(q))) and len(q) >= 1, cmd[:120]
            assert q[0][2] == item_ptr[p] and q[-1][3] == item_ptr[p + 1], cmd[:120]
            assert all(a[3] == b[2] for a, b in zip(q[:-1], q[1:])) and all(c[2] <= c[3] for c in q), cmd[:120]
            assert all(c[1] == (len(q) > 1) for c in q), cmd[:120]
        shared = any(len(q) > 1 for q in per_panel)
        assert got["shared"] == [int(shared)]
        if shared:
            key = (lambda c: (c[4], c[0])) if plain else (lambda c: (c[4] >> 3, c[0], c[4] & 7))
        else:
            key = lambda c: c[0]
        assert chunks == sorted(chunks, key=key), cmd[:120]
        total, nitems = (P if P >= slots else 8 * slots), item_ptr[-1]
        if nitems >= total:
            owed = [(item_ptr[p + 1] - item_ptr[p]) * total // nitems for p in range(P)]       # floor(share), in integers
            assert n == max(total, sum(max(k, 1) for k in owed)), cmd[:120]
            if min(owed) >= 1:
                assert n == total, cmd[:120]
                exact += 1
    assert exact >= 12          # P <, ==, > slots with equal panels, both slot counts, both orders


def test_every_long_row_has_one_owner(results):
    for cmd, (cands, cap_rows), got in _with(results, "long"):
        nlong = min(len(cands), cap_rows)
        rows, own_first, owner_of, lptr = got["rows"], got["own_first"], got["owner_of"], got["lptr"]
        assert len(rows) == len(owner_of) == nlong and len(lptr) == nlong + 1 and len(own_first) == M.K_LONG_OWNERS + 1
        assert own_first[0] == 0 and own_first[-1] == nlong and all(a <= b for a, b in zip(own_first[:-1], own_first[1:]))
        length = dict(cands)
        shortest_taken = min((length[r] for r in rows), default=0)
        assert len(set(rows)) == nlong and all(length[r] <= shortest_taken for r in length if r not in rows)      # the longest ones
        for w in range(M.K_LONG_OWNERS):
            blk = rows[own_first[w]:own_first[w + 1]]
            assert blk == sorted(blk) and all(o == w for o in owner_of[own_first[w]:own_first[w + 1]])
            assert len(blk) in (nlong // M.K_LONG_OWNERS, -(-nlong // M.K_LONG_OWNERS))
        assert lptr[0] == 0 and all(lptr[i + 1] - lptr[i] == length[rows[i]] for i in range(nlong))


def test_generation_cuts_add_no_generation(results):
    """plan_generation_cuts (products in parts, products with host vectors): the cuts run from 0 to nunits and never back, every
    cut inside the launch is a multiple of `slots`, the parts' generations ceil(len / slots) add up to those of the undivided
    launch, and exactly min(nparts, generations) parts are not empty"""
    for cmd, (nunits, slots, nparts), got in _with(results, "cuts"):
        units = got["units"]
        if GENERATION_CUTS[(nunits, slots, nparts)] is not None:
            assert units == GENERATION_CUTS[(nunits, slots, nparts)], cmd
        gens = -(-nunits // slots)
        lens = [b - a for a, b in zip(units[:-1], units[1:])]
        assert len(units) == nparts + 1 and units[0] == 0 and units[-1] == nunits and all(n >= 0 for n in lens), cmd
        assert all(u % slots == 0 for u in units[1:-1] if u < nunits), cmd
        assert sum(-(-n // slots) for n in lens) == gens, cmd
        assert sum(n > 0 for n in lens) == min(nparts, gens), cmd


def test_padded_segments_are_even_and_consistent(results):
    for cmd, (hs, B), got in _with(results, "segments"):
        hp, hseg, hsh, K = got["hp"], got["hseg"], got["hsh"], M.K_LONG_OWNERS
        assert got["ok"] == [1] and hp[0] == 0
        for b in range(B):
            seg = hseg[b * (K + 1):(b + 1) * (K + 1)]
            assert seg[0] == 0 and seg[K] == hp[b + 1] - hp[b]
            for w in range(K):
                sg, padded = b * K + w, seg[w + 1] - seg[w]
                count = hs[sg + 1] - hs[sg]
                assert padded % 2 == 0 and 0 <= padded - count <= 1, cmd[:80]
                assert hsh[sg] == hp[b] + seg[w] - hs[sg]                                # padded position - sorted position
