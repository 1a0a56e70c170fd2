"""The narrowing schedule of fs_pcgn / fs_pcgn_lambdas under option "pcgn_compact" (libfastsparse_amd/csrc/fs_pcgn_plan.h) on the CPU
alone.

tests/pcgn_plan_driver.cpp -- a stand-alone program around fs_pcgn_plan.h -- is compiled with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer and run ONCE as a child process on every case below.  Asserted:
  1. its segments equal tests/_pcgn_plan_model.py's (written from the header's text) on every k in {1, 2, 3, 4, 5, 8, 16, 17, 32},
     on seeded count vectors with columns frozen from the start and capped ones, on full ladders and ladders with rungs removed;
  2. three cases checked by hand (counts from tests/_pcgn_lambdas_model.py on the two recipe ladders);
  3. what the solve relies on, stated without the model: widths never grow and are usable rungs, a panel holds its columns, every
     column of a segment was live two iterations before the segment starts, at most five repacks.
"""
import os
import random
import shutil
import subprocess

import pytest

import _pcgn_plan_model as PM

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "libfastsparse_amd", "csrc")
KS = (1, 2, 3, 4, 5, 8, 16, 17, 32)
PER_K = 40
HAND = [  # (k, usable widths, counts, frozen0, cap, segments as (first, width))
    (8, (4, 2, 1), [19, 18, 16, 14, 10, 6, 4, 2], [0] * 8, 200, [(0, 8), (12, 4), (18, 2)]),
    (2, (1,), [19, 2], [0, 0], 200, [(0, 2), (4, 1)]),
    (8, (4, 2, 1), [22, 22, 22, 21, 20, 17, 14, 9], [0] * 8, 200, [(0, 8), (22, 4)]),
]


def _ladders(k):
    full = [w for w in PM.RUNGS if w < k]
    out = [full, []]
    for drop in range(len(full)):
        out.append(full[:drop] + full[drop + 1:])
    if len(full) >= 3:
        out.append(full[::2])
        out.append(full[-1:])
    return out


def _counts(rng, k, cap):
    """counts of every shape: spread wide, bunched, tails of one or two columns; some columns frozen from the start, some at the cap"""
    kind = rng.randrange(5)
    if kind == 0:
        c = [rng.randrange(0, cap + 1) for _ in range(k)]
    elif kind == 1:
        top = rng.randrange(1, cap + 1)
        c = [max(0, top - rng.randrange(3)) for _ in range(k)]
    elif kind == 2:
        c = [rng.randrange(0, 4) for _ in range(k)]
        for j in rng.sample(range(k), min(k, rng.randrange(1, 3))):
            c[j] = rng.randrange(cap // 2, cap + 1)
    elif kind == 3:
        c = sorted((int(cap * (0.5 ** rng.randrange(6))) for _ in range(k)), reverse=True)
    else:
        c = [cap] * k
    frozen = [int(rng.random() < (1.0 if kind == 4 and rng.random() < 0.3 else 0.15)) for _ in range(k)]
    c = [0 if f else v for v, f in zip(c, frozen)]
    return c, frozen


def _cases():
    rng = random.Random(20250114)
    out = [(k, tuple(u), c, f, cap) for k, u, c, f, cap, _ in HAND]
    for k in KS:
        for _ in range(PER_K):
            cap = rng.choice((1, 2, 3, 5, 24, 60))
            counts, frozen = _counts(rng, k, cap)
            out.append((k, tuple(rng.choice(_ladders(k))), counts, frozen, cap))
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case through the sanitized driver, in one child process"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/pcgn_plan_driver.cpp")
    cases = _cases()
    exe = str(tmp_path_factory.mktemp("pcgn_plan") / "pcgn_plan_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(HERE, "pcgn_plan_driver.cpp"), "-o", exe], check=True)
    lines = [" ".join(str(v) for v in [k, PM.usable_bits(u), cap] + c + f) for k, u, c, f, cap in cases]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got = []
    for line in run.stdout.splitlines():
        key, *vals = line.split()
        if key == "case":
            got.append({})
        else:
            got[-1][key] = [int(v) for v in vals]
    assert len(got) == len(cases)
    return [(case, [tuple(g["segments"][i:i + 3]) for i in range(0, len(g["segments"]), 3)], g["rungs"]) for case, g in zip(cases, got)]


def test_the_cases_cover_what_the_issue_names(results):
    assert {c[0] for c, _, _ in results} == set(KS)
    assert len(results) >= 300
    narrowed = sum(len(s) > 1 for _, s, _ in results)
    frozen = sum(any(c[3]) for c, _, _ in results)
    all_frozen = sum(all(c[3]) for c, _, _ in results)
    removed = sum(set(c[1]) != {w for w in PM.RUNGS if w < c[0]} for c, _, _ in results)
    before_first = sum(len(s) == 1 and s[0][1] < c[0] for c, s, _ in results)
    capped = sum(max(c[2]) == c[4] for c, _, _ in results)
    assert min(narrowed, frozen, removed, capped) > 40 and all_frozen > 3 and before_first > 3, (narrowed, frozen, all_frozen, removed, before_first, capped)


def test_the_rungs(results):
    for (k, *_), _, rungs in results:
        assert rungs == [PM.rung(L) for L in range(1, k + 1)]
        assert all(w >= L and (w == 1 or w // 2 < L) and w & (w - 1) == 0 for L, w in enumerate(rungs, 1))


def test_every_plan_equals_the_model(results):
    for (k, usable, counts, frozen, cap), segs, _ in results:
        assert segs == PM.plan(k, usable, counts, frozen, cap), (k, usable, counts, frozen, cap)


def test_the_hand_checked_cases(results):
    for (k, usable, counts, frozen, cap, want), (_, segs, _) in zip(HAND, results):
        assert [(a, w) for a, w, _ in segs] == want, (counts, segs)
    # the columns each panel holds: the longest ones, in original numbering
    assert [m for _, _, m in results[0][1]] == [0xFF, 0b1111, 0b11]
    assert [m for _, _, m in results[1][1]] == [0b11, 0b01]
    assert [m for _, _, m in results[2][1]] == [0xFF, 0b1111]


def test_schedule_properties(results):
    for (k, usable, counts, frozen, cap), segs, _ in results:
        what = (k, usable, counts, frozen, cap, segs)
        assert segs[0][0] == 0 and len(segs) <= 6, what
        if len(segs) > 1 or segs[0][1] == k:
            assert segs[0][1] in (k,) + tuple(usable), what
        if segs[0][1] == k:
            assert segs[0][2] == PM.all_columns(k), what
        firsts, widths = [a for a, _, _ in segs], [w for _, w, _ in segs]
        assert firsts == sorted(set(firsts)) and widths == sorted(set(widths), reverse=True), what
        live0 = [not f for f in frozen]
        last = max((min(c, cap - 1) for c, l in zip(counts, live0) if l), default=-1)
        for i, (first, width, mask) in enumerate(segs):
            cols = [j for j in range(k) if mask >> j & 1]
            assert len(cols) <= width and mask < (1 << k), what
            if width < k:
                assert width in usable and first <= last, what
                # the columns that were live when the host last looked: after iteration first - 2
                assert cols == [j for j in range(k) if live0[j] and (first < 2 or counts[j] > first - 2)], what
                # the narrowest usable rung that holds them
                assert width == min(w for w in usable if w >= len(cols)), what
