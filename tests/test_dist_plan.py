"""The exchange layout of the sharded products (libfastsparse_amd/csrc/fs_dist_plan.h) on the CPU alone.

tests/dist_plan_driver.cpp -- a stand-alone program around fs_dist_plan.h -- is compiled with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer and run ONCE as a child process on every case below.  Three things are asserted:
  1. its outputs equal tests/_dist_plan_model.py's, element for element;
  2. what the engine of fs_dist.hip relies on, stated without the model, for the overlapped and the whole-shard layout;
  3. the exchange played in numpy -- padded all-gathers part by part, then the unpack from the table -- leaves every rank
     with the whole vector.
"""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import _dist_plan_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "libfastsparse_amd", "csrc")
RANKS = (1, 2, 3, 8)
COLUMNS = (1, 2, 4, 32)
PARTS = (1, 4, 7, 16)
BOUNDS = ("random", "empty first rank", "empty last rank", "one rank owns every row", "no rows")
SCALARS = ("n", "k", "np", "real", "max_rows", "nseg", "nseg1", "max_seg", "pad_rows", "local_rows", "window_rows", "busy", "whole_at")


def _bounds(rng, n, kind):
    if kind == "no rows":
        return [0] * (n + 1)
    if kind == "one rank owns every row":
        owner, nrow = rng.randrange(n), rng.randrange(1, 300)
        return [0 if r <= owner else nrow for r in range(n + 1)]
    sizes = [rng.choice((0, 1, 2, 17, 100, 257)) if rng.random() < 0.5 else rng.randrange(0, 300) for _ in range(n)]
    if kind == "empty first rank":
        sizes[0] = 0
    if kind == "empty last rank":
        sizes[-1] = 0
    return [sum(sizes[:r]) for r in range(n + 1)]


def _cuts(rng, n, np_, bounds):
    """row cuts of every rank: one part empty on ALL ranks (np > 1), further parts empty on some ranks, sometimes all rows in one part"""
    dead = rng.randrange(np_) if np_ > 1 else -1
    cut = []
    for r in range(n):
        nl = bounds[r + 1] - bounds[r]
        w = [0 if p == dead or rng.random() < 0.3 else rng.randrange(1, 10) for p in range(np_)]
        if rng.random() < 0.2 or not any(w):
            w = [0] * np_
            w[rng.choice([p for p in range(np_) if p != dead])] = 1
        at = [nl * sum(w[:p]) // sum(w) for p in range(np_ + 1)]
        cut.append(at)
    return cut


def _cases():
    rng = random.Random(20240911)
    out = []
    for n in RANKS:
        for k in COLUMNS:
            for np_ in PARTS:
                for kind in BOUNDS:
                    bounds = _bounds(rng, n, kind)
                    cut = _cuts(rng, n, np_, bounds)
                    line = " ".join(str(v) for v in [n, k, np_] + bounds + [c for row in cut for c in row])
                    out.append((line, (n, k, np_, bounds, cut, kind)))
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case through the sanitized driver, in one child process"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/dist_plan_driver.cpp")
    cases = _cases()
    exe = str(tmp_path_factory.mktemp("dist_plan") / "dist_plan_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(HERE, "dist_plan_driver.cpp"), "-o", exe], check=True)
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
    return [(meta, g) for (_, meta), g in zip(cases, got)]


def _layouts(got):
    """((dst, src, cnt) of the overlapped layout, (dst, src, cnt) of the whole-shard layout), as the table holds them"""
    s = dict(zip(SCALARS, got["scalars"]))
    t, a, b = np.array(got["table"], np.int64), s["nseg"], s["nseg1"]
    assert len(t) == 3 * (a + b) and s["whole_at"] == 3 * a
    return s, (t[:a], t[a:2 * a], t[2 * a:3 * a]), (t[3 * a:3 * a + b], t[3 * a + b:3 * a + 2 * b], t[3 * a + 2 * b:])


def test_the_cases_cover_what_the_issue_names(results):
    seen = {(n, k, np_, kind) for (n, k, np_, _, _, kind), _ in results}
    assert seen == {(n, k, np_, kind) for n in RANKS for k in COLUMNS for np_ in PARTS for kind in BOUNDS}
    some = all_ranks = real = unreal = 0
    for (n, k, np_, bounds, cut, kind), got in results:
        rows = np.diff(np.array(cut), axis=1)
        some += bool(((rows == 0).any(axis=0) & (rows > 0).any(axis=0)).any())       # a part empty on some ranks only
        all_ranks += bool(np_ > 1 and (rows == 0).all(axis=0).any())
        real += got["scalars"][3]
        unreal += not got["scalars"][3]
    assert some > 50 and all_ranks > 50 and real > 50 and unreal > 50


def test_every_output_equals_the_model(results):
    for (n, k, np_, bounds, cut, kind), got in results:
        assert got == M.plan_exchange(n, k, bounds, cut), (n, k, np_, kind)


def test_k1_is_the_single_vector_layout_in_rows(results):
    """with k = 1 doubles are rows: the table of a k-column plan is the k = 1 table of the same cuts times k"""
    for (n, k, np_, bounds, cut, kind), got in results:
        one = M.plan_exchange(n, 1, bounds, cut)
        assert got["table"] == [v * k for v in one["table"]] and got["maxc"] == one["maxc"] and got["off"] == one["off"]
        assert got["scalars"][4:7] == one["scalars"][4:7] and got["scalars"][7] == one["scalars"][7] * k and got["scalars"][8:] == one["scalars"][8:]


def test_layout_properties(results):
    for (n, k, np_, bounds, cut, kind), got in results:
        s, parts, whole = _layouts(got)
        nrow, maxc, off = bounds[-1], got["maxc"], got["off"]
        for dst, src, cnt in (parts, whole):
            assert np.all(cnt > 0)
            # the destinations tile [0, nrow * k) exactly once
            order = np.argsort(dst, kind="stable")
            edges = np.concatenate([[0], (dst + cnt)[order]])
            assert np.array_equal(dst[order], edges[:-1]) and edges[-1] == nrow * k, (n, k, np_, kind)
            # the sources are disjoint and inside the padded size
            order = np.argsort(src, kind="stable")
            assert np.all((src + cnt)[order][:-1] <= src[order][1:]) and np.all(src >= 0) and np.all(src + cnt <= s["pad_rows"] * k)
        # segment (p, r) is where an all-gather of maxc[p] * k doubles into pad + off[p] * k puts rank r
        want = [(off[p] + r * maxc[p]) * k for p in range(np_) for r in range(n) if cut[r][p + 1] > cut[r][p]]
        assert list(parts[1]) == want and s["max_seg"] == (max(parts[2]) if len(parts[2]) else 0)
        assert list(whole[1]) == [r * s["max_rows"] * k for r in range(n) if bounds[r + 1] > bounds[r]]
        # every send window stays inside the local buffer, every part's region inside the padded one
        assert all(cut[r][p] + maxc[p] <= 2 * s["max_rows"] for r in range(n) for p in range(np_))
        assert s["local_rows"] == 2 * s["max_rows"] + 1 and s["window_rows"] == s["max_rows"]
        assert off[np_] <= s["pad_rows"] and n * s["max_rows"] <= s["pad_rows"]
        assert s["real"] == int(s["busy"] > 1) and s["busy"] == max(sum(b > a for a, b in zip(c[:-1], c[1:])) for c in cut)


def test_the_exchange_played_in_numpy(results):
    """every rank's local output holds its rows' global indices (poison behind them); the padded all-gathers part by part and
    the unpack from the table leave arange(nrow * k) on every rank -- and so does the whole-shard layout"""
    for (n, k, np_, bounds, cut, kind), got in results:
        s, parts, whole = _layouts(got)
        nrow, maxc, off = bounds[-1], got["maxc"], got["off"]
        local = []
        for r in range(n):
            buf = np.full(s["local_rows"] * k, -1, np.int64)
            buf[:(bounds[r + 1] - bounds[r]) * k] = np.arange(bounds[r] * k, bounds[r + 1] * k)
            local.append(buf)

        def gather(pad, first_row, window_rows, at):
            """one all-gather: `window_rows * k` doubles from row at(r) of every rank's local output, to row first_row of pad"""
            count = window_rows * k
            for r in range(n):
                piece = local[r][at(r) * k:at(r) * k + count]
                assert len(piece) == count                                  # the send window is inside the local buffer
                lo = first_row * k + r * count
                assert lo + count <= len(pad)
                pad[lo:lo + count] = piece

        def unpack(pad, table):
            out = np.full(nrow * k, -3, np.int64)
            for d, a, c in zip(*table):
                out[d:d + c] = pad[a:a + c]
            return out

        for d in range(n):                   # every rank receives the same calls: played once per destination all the same
            pad = np.full(s["pad_rows"] * k, -2, np.int64)
            for p in range(np_):
                gather(pad, off[p], maxc[p], lambda r: cut[r][p])
            assert np.array_equal(unpack(pad, parts), np.arange(nrow * k)), (n, k, np_, kind, d)
            pad = np.full(s["pad_rows"] * k, -2, np.int64)
            gather(pad, 0, s["window_rows"], lambda r: 0)
            assert np.array_equal(unpack(pad, whole), np.arange(nrow * k)), (n, k, np_, kind, d)
