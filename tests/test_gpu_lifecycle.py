"""Long-lived handles on the real library: random operation walks with every vector inside guard zones (tests/_lifecycle.py).

The other GPU tests run one fixed script on a fresh handle.  Here a handle lives through a walk of legal calls -- products of every
kind, prepare / release, release_csr / restore_csr, option flips, stream changes, neighbours created and destroyed -- and after
every operation the guards of all vectors are untouched, the inputs unchanged, the outputs exact, the statuses what the header
promises and the bookkeeping what the debug hooks saw.  Two solver pairs (A, At) live through the same walks and through
fs_gram_diag, fs_cg, fs_cg2, fs_pcg, fs_mscg, fs_pcgn, fs_pcgn_lambdas and fs_mscgn, with options "pcgn_kernel" and "pcgn_compact"
among the flips (the segments of a narrowing solve against the plan model on the widths usable at that moment),
half of the solves on work space that was poisoned just before (see tests/_lifecycle.py).  tests/test_lifecycle_model.py shows on a numpy stand-in that these checks catch the faults they are meant
for, and that the seeds used here reach every operation."""
import ctypes as C

import numpy as np
import pytest

import _cg_model as M
import _exact as E
import _lifecycle as LC
from _exact import PATHS
from _gpu import options

pytestmark = pytest.mark.gpu

SEEDS = (1, 2)
STEPS = 150
SET_NAMES = LC.GPU_SET_NAMES           # (why these two: see there)
COPIES = list(PATHS) + [LC.AUTO]
# the mid-size set with panels of 32 rows: more generations of resident workgroups than the largest nparts
POISON = {"seen": 0, "probed": 0, "poisoned": 0}       # what the probes of poison_heap saw, summed over this module's walks
SMALL_PANELS = {"two-pass, panels of 32 rows": (dict(binning=2, ldsx=0, tiling=0, bin_rows=32), "two-pass"),
                "lds-staged, panels of 32 rows": (dict(ldsx=2, binning=0, tiling=0, tile_rows=32), "lds-staged")}


@pytest.fixture(scope="module")
def backend():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return LC.HipBackend(dict(PATHS, **SMALL_PANELS), options)


@pytest.fixture(scope="module")
def mid():
    d = LC.mid_size()
    return d, LC.refs_of(d, nc=2, ata_cols=0)


@pytest.mark.parametrize("copy", COPIES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_walks_are_exact_and_stay_inside_their_vectors(backend, name, copy):
    d = LC.data_sets()[name]
    for seed in SEEDS:
        w = LC.run_walk(backend, d, copy, seed, steps=STEPS, copies=COPIES)
        assert sum(w.counts["ops"].values()) == STEPS
        _count_poison(w)


def _count_poison(w):
    for k in POISON:
        POISON[k] += w.counts["poison_" + k if k != "poisoned" else k]


def test_solvers_on_poisoned_work_space(backend):
    """every solver right behind poison_heap: freed device memory of the sizes the solve is about to ask for holds a tagged NaN, so a
    work vector (r, p, q, tmp, part, red, st, dinv / s, the directions of fs_mscg, the partials and scalars of fs_pcgn and
    fs_pcgn_lambdas, the direction panels, partials and 9344 scalars of fs_mscgn) that is read before it is written puts that tag
    into x.  The exact family in the default mode (both twins: every fs_pcg start and preconditioner, the ladders with ldx > F,
    fs_pcgn and fs_pcgn_lambdas at every k with columns frozen from the start, fs_mscgn at every k and ladder, packed and padded
    panels), the general system under strict_order against the models, state included.  The bar is the walks': exact bits"""
    w = LC.Walk(backend, LC.data_sets()["wide_range_odd"], LC.AUTO, seed=11, steps=0, copies=COPIES)
    with w.session():
        w.create(first=True)
        for valued in (False, True):
            pair = w.create_pair("exact", valued=valued)
            cases = LC.exact_cases(pair.ps.fam)
            nth = {}
            for solver, what, _ in cases:
                j = nth[solver] = nth.get(solver, -1) + 1
                if solver in ("pcgn", "pcgn_lambdas") and (j + valued) % 5:      # (a fifth of the 54 panels per twin: every k is met)
                    continue
                w.step += 1
                rc, _ = w.exact_solve(pair.A, solver, poison=True, pick=j)
                assert rc == LC.FS_OK, what
                for h in (pair.A, pair.At):
                    w.recover(h)
            w.step += 1
            w.op_gram_diag(pair.A)
        exact = pair
        pair = w.create_pair("general")
        for i in range(len(LC.strict_cases(pair.ps))):
            w.step += 1
            assert w.op_solve_strict(pair.A, pick=i, poison=True) == LC.FS_OK
            for h in (pair.A, pair.At):
                w.recover(h)
        met = {sv: {kw["b"].size // pair.ps.s.ncol for s2, _, kw in LC.strict_cases(pair.ps) if s2 == sv} for sv in LC.K_COLUMNS}
        assert met == {"pcgn": {3, 5}, "pcgn_lambdas": {3, 5}, "mscgn": {1, 3}} and w.counts["poisoned"] >= 100, (met, w.counts["poisoned"])
        assert w.counts["solves"]["pcgn_lambdas"] >= 6 and w.counts["solves"]["mscgn"] >= 6, w.counts["solves"]
        print(f"poisoned solves: {w.counts['solves']}")
        # option "pcgn_compact": solves that really repack (LC.repacking_cases; the choice is checked on the CPU with the models), on
        # poisoned work space -- the narrow panels X, R, P at w1, X at w2 and the 512 scalars are bare allocations whose padding
        # columns must read +0.0.  run_solver holds the segments against the plan model
        assert w.counts["repacked"] == 0
        w.flip("pcgn_compact", 1)
        before = dict(w.counts["solves"])
        for solver, i, what in LC.repacking_cases(pair.ps):
            w.step += 1
            assert w.op_solve_strict(pair.A, pick=i, poison=True) == LC.FS_OK, what
        for solver, j, what in LC.repacking_cases(exact.ps):
            w.step += 1
            rc, _ = w.exact_solve(exact.A, solver, poison=True, pick=j)
            assert rc == LC.FS_OK, what
        ran = sum(w.counts["solves"][sv] - before[sv] for sv in LC.NARROWING)
        w.flip("pcgn_compact", 0)
        print(f"pcgn_compact = 1: {w.counts['repacked']} of {ran} poisoned fs_pcgn / fs_pcgn_lambdas solves repacked")
        assert w.counts["repacked"] == ran >= 6, (w.counts["repacked"], ran)
    _count_poison(w)
    print(f"poison probes: {w.counts['poison_seen']} of {w.counts['poison_probed']} doubles still held the poison")


def test_solver_work_space_is_given_back(backend):
    """one pair, no walk: after two warm-up solves, 50 fs_pcgn solves (k = 32, Jacobi, F = 2000) and 50 fs_mscg solves (m = 16) leave
    free device memory no lower than by ONE solve's work space (the header's formula: 3 k F + k N + F + 2048 k + 512 doubles, about
    2 MB; a leak of a solve's work space per solve would be a hundred times that).  CgFlags' pinned memory and events cannot be seen
    in free memory: for them 1000 solves that are done before their first iteration (b = 0: no product) all return FS_OK"""
    import torch
    from libfastsparse_amd import capi
    ps = LC.pair_system("exact")
    fam, s, mem = ps.fam, ps.s, backend.mem
    (arp, acc, _), (trp, tcc, _) = ps.a_csr, ps.t_csr
    A = capi.Matrix.from_csr(s.nrow, s.ncol, mem.const(arp), mem.const(acc), None)
    At = capi.Matrix.from_csr(s.ncol, s.nrow, mem.const(trp), mem.const(tcc), None)
    st = capi.current_stream()
    k, lams = 32, fam.ladders["m16"]
    B, b = mem.const(fam.panel(k)), mem.const(s.b)
    X, Xm, x = torch.empty_like(B), torch.empty((16, s.ncol), dtype=torch.float64, device="cuda"), torch.empty_like(b)
    zero = torch.zeros_like(b)
    want_n, want_m = mem.const(fam.panel(k) / fam.c), mem.const(np.stack([s.b / (fam.d + l) for l in lams]))

    def both():
        infos = capi.pcgn(A, At, X, B, s.lam, s.tol, precond=capi.FS_PRECOND_JACOBI, stream=st)
        assert all(i.converged == 1 for i in infos) and mem.eq(X, want_n)
        infos = capi.mscg(A, At, Xm, b, lams, s.tol, stream=st)
        assert all(i.converged == 1 for i in infos) and mem.eq(Xm, want_m)

    both()
    both()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(50):
        both()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    one_solve = 8 * (3 * k * s.ncol + k * s.nrow + s.ncol + 2048 * k + 512)
    print(f"free device memory: {free0} bytes after the warm-up, {free1} after 100 solves more; one solve's work space {one_solve} bytes")
    assert free0 - free1 <= one_solve, (free0, free1, one_solve)
    for _ in range(1000):
        info = capi.pcg(A, At, x, zero, s.lam, s.tol, precond=capi.FS_PRECOND_NONE, stream=st)
        assert info.converged == 1 and info.iterations == 0
    assert not x.any().item()
    torch.cuda.synchronize()
    free2 = torch.cuda.mem_get_info()[0]
    print(f"free device memory after 1000 solves without an iteration: {free2} bytes")
    assert free0 - free2 <= one_solve, (free0, free2, one_solve)


@pytest.mark.parametrize("copy", list(SMALL_PANELS))
def test_products_in_parts_survive_plan_eviction(backend, mid, copy):
    """the mid-size set, really cut (asserted): nparts 2..12 in random order on A and on A', and again in reverse -- eleven plans
    through a cache of eight, with `reproducible` flipped half way so that one nparts owns two -- every product exact after every
    part, and the rows fs_spmv_part_rows reports for an nparts the same before and after its plan was pushed out"""
    d, _ = mid
    w = LC.Walk(backend, d, copy, seed=5, steps=0, kmax=2, nc=2, ata_cols=0)
    with w.session():
        H = w.create(first=True, with_t=True, borrow=False)
        rng = np.random.default_rng(5)
        for side in (0, 1):
            n = H.refs.n_out[side]
            first = {}
            order = [int(v) for v in rng.permutation(np.arange(2, 13))]
            for i, nparts in enumerate(order + order[::-1]):
                w.step = i
                if i == len(order) // 2:
                    w.flip("reproducible", 1)
                if i == len(order):
                    w.flip("reproducible", 0)
                rows = H.A.part_rows(nparts, bool(side))
                assert any(0 < r < n for r in rows), (copy, side, nparts, rows, "the product is not cut: the set has too few panels")
                assert first.setdefault(nparts, rows) == rows, (copy, side, nparts, first[nparts], rows)
                assert w.one_product_in_parts(H, side, 1, nparts) == LC.FS_OK
        # one nparts owns a plan per kernel: first met under strict_order (the chunk-streaming kernel: everything with part 0), then
        # under the default options it must get the cuts of the kept copy, not the plan filed under the same nparts
        for side, nparts in ((0, 13), (1, 14)):
            w.step = 50 + side
            w.flip("strict_order", 1)
            rows = H.A.part_rows(nparts, bool(side))
            assert rows == [0] + [H.refs.n_out[side]] * nparts, (copy, side, rows)
            assert w.one_product_in_parts(H, side, 1, nparts) == LC.FS_OK
            w.flip("strict_order", 0)
            rows = H.A.part_rows(nparts, bool(side))
            assert any(0 < r < H.refs.n_out[side] for r in rows), (copy, side, nparts, rows, "the cuts of another kernel's plan")
            assert w.one_product_in_parts(H, side, 1, nparts) == LC.FS_OK
        assert w.op_prepare(H, 2, 0) == LC.FS_OK
        for i, nparts in enumerate((3, 12, 5, 12, 2)):
            w.step = 100 + i
            assert w.one_product_in_parts(H, 0, 2, nparts) == LC.FS_OK
        if SMALL_PANELS[copy][1] == "two-pass":
            rows = H.A.part_rows(12, False, 2)
            assert any(0 < r < d.nrow for r in rows), (rows, "the 2-column sweep is not cut")


@pytest.mark.parametrize("copy", ["two-pass", "lds-staged"])
def test_release_prepared_k_by_k_gives_everything_back(backend, copy):
    """prepare for several k, release them one by one in another order: products exact in between, and once the last is gone
    fs_matrix_device_bytes()[2] is 0 again (the column-major scratch of the LDS-staged copy goes with the last k that used it)"""
    d = LC.data_sets()["subnormal"]
    w = LC.Walk(backend, d, copy, seed=9, steps=0)
    with w.session():
        H = w.create(first=True, with_t=True, borrow=False)
        assert H.A.device_bytes()[2] == 0
        for i, k in enumerate((3, 5, 8, 2, 4)):
            w.step = i
            assert w.op_prepare(H, k, i & 1) == LC.FS_OK
            w.op_spmm(H, i & 1)
        assert H.A.device_bytes()[2] > 0
        for i, k in enumerate((8, 5, 4, 3, 2)):
            w.step = 10 + i
            w.op_release_prepared(H, k)
            w.op_spmm(H, i & 1)
        assert H.A.device_bytes()[2] == 0, H.A.device_bytes()


def test_first_fixed_order_product_late_in_life(backend):
    """the two-byte row ids a one-byte two-pass copy writes on its first fixed-order product: after many default products the handle
    meets `reproducible`, then a solver's scope (fs_cg on a system whose every sum is exact: x = b / 2^e at iteration 0), then the
    default mode again.  Exact each time; fs_matrix_device_bytes grows once per copy, by at most 2 bytes per padded entry, and the
    growth is there right after the first such product"""
    import torch
    from libfastsparse_amd import capi
    L = backend.L
    s = M.exact_system(m=3, lam=1.0, F=2000, seed=23)
    (arp, acc, _), (trp, tcc, _) = s.a_csr(), s.t_csr_sorted()
    rows = np.repeat(np.arange(s.nrow), np.diff(arp))
    mem = backend.mem
    xs = [s.b] + [s.b * 2.0 ** j * np.where(np.random.default_rng(j).uniform(size=s.ncol) < 0.5, -1.0, 1.0) for j in range(1, 6)]
    us = [np.random.default_rng(50 + j).integers(-512, 513, s.nrow).astype(np.float64) for j in range(6)]
    ys = [E.spmv(s.nrow, rows, acc, None, x) for x in xs]
    zs = [E.spmv_t(s.ncol, rows, acc, None, u) for u in us]
    with options(**PATHS["two-pass one-byte"][0]):
        A = capi.Matrix.from_csr(s.nrow, s.ncol, mem.const(arp), mem.const(acc), None)
        At = capi.Matrix.from_csr(s.ncol, s.nrow, mem.const(trp), mem.const(tcc), None)
    padded = []
    for X in (A, At):
        assert X.kernel_name() == "two-pass" and L.fs_debug_two_pass_rows8(X.h, 0) >= 0, "not a one-byte two-pass copy"
        out8 = (C.c_ulonglong * 8)()
        assert L.fs_debug_two_pass_layout(X.h, 0, out8) == 0
        padded.append(int(out8[5]))
    gin = {X: LC.Guarded(mem, f"x of {n}", max(s.nrow, s.ncol)) for X, n in ((A, "A"), (At, "At"))}
    gout = {X: LC.Guarded(mem, f"y of {n}", max(s.nrow, s.ncol)) for X, n in ((A, "A"), (At, "At"))}
    st = capi.current_stream()
    count = [0]

    def product(X, what):
        j = count[0] % 6
        count[0] += 1
        x, want = (xs[j], ys[j]) if X is A else (us[j], zs[j])
        mem.put(gin[X].place(x.size, count[0] & 1), x)
        mem.fill_bits(gout[X].place(want.size, (count[0] >> 1) & 1), LC.PREFILLS["nan"])
        X.spmv(gout[X].view, gin[X].view, st)
        got = mem.get(gout[X].view)
        assert E.bits_equal(got, want), (what, count[0], E.first_mismatch(got, want))
        assert gin[X].guards_ok() and gout[X].guards_ok() and mem.eq(gin[X].view, mem.const(x)), (what, count[0])

    for _ in range(12):
        product(A, "default, early in life")
        product(At, "default, early in life")
    before = (A.device_bytes(), At.device_bytes())
    with options(reproducible=1):
        product(A, "the first fixed-order product")
        grown = A.device_bytes()
        assert 0 < grown[1] - before[0][1] <= 2 * padded[0] and grown[0] == before[0][0] and grown[2] == before[0][2], (before[0], grown, padded)
        for _ in range(3):
            product(A, "reproducible")
        assert A.device_bytes() == grown, "the copy grew a second time"
    assert At.device_bytes() == before[1]
    b = mem.const(s.b)
    x = LC.Guarded(mem, "x of fs_cg", s.ncol)
    mem.fill_bits(x.place(s.ncol, 1), LC.PREFILLS["nan"])
    it = C.c_int(-1)
    capi.check(L.fs_cg(A.h, At.h, x.view.data_ptr(), b.data_ptr(), s.lam, s.tol, C.byref(it), st), "fs_cg")
    torch.cuda.synchronize()
    assert it.value == 0 and E.bits_equal(mem.get(x.view), s.b / (3 + s.lam)) and x.guards_ok(), (it.value, E.first_mismatch(mem.get(x.view), s.b / (3 + s.lam)))
    grown_t = At.device_bytes()
    assert 0 < grown_t[1] - before[1][1] <= 2 * padded[1], (before[1], grown_t, padded)          # the solver's scope met A' first
    assert A.device_bytes() == grown
    for _ in range(6):
        product(A, "default again")
        product(At, "default again")
    assert A.device_bytes() == grown and At.device_bytes() == grown_t


@pytest.mark.parametrize("copy", list(PATHS))
def test_captured_walk_replays(backend, copy):
    """spmv, spmv_t, spmm k = 2 and 8, ata captured once on the test's stream, replayed three times with new right-hand sides copied
    into the captured input vectors: guards and exact bits after every replay (a replay that serves the rows of the capture, or of
    the replay before, fails: the columns change every time)"""
    import torch
    from libfastsparse_amd import capi
    d = LC.data_sets()["subnormal_pattern"]
    r = LC.refs_of(d)
    mem = backend.mem
    s = torch.cuda.Stream()
    with options(**PATHS[copy][0]):
        A = capi.Matrix.from_csr(d.nrow, d.ncol, mem.const(d.rp), mem.const(d.cols), None)
        A.build_transpose(capi.current_stream())
        for k in (2, 8):
            A.prepare(k, capi.current_stream())
    torch.cuda.synchronize()
    # (name, side of the input, side of the output, k)
    calls = [("spmv", 0, 0, 1), ("spmv_t", 1, 1, 1), ("spmm2", 0, 0, 2), ("spmm8", 0, 0, 8), ("spmm_t2", 1, 1, 2), ("ata", 0, 1, 1)]
    with torch.cuda.stream(s):
        gi, go = {}, {}
        for i, (name, si, so, k) in enumerate(calls):
            gi[name] = LC.Guarded(mem, f"input of {name}", r.n_in[si] * k)
            go[name] = LC.Guarded(mem, f"output of {name}", r.n_out[so] * k)
            gi[name].place(r.n_in[si] * k, i & 1)
            go[name].place(r.n_out[so] * k, (i >> 1) & 1)
        tmp = LC.Guarded(mem, "tmp of ata", d.nrow)
        tmp.place(d.nrow, 1)

        def launch():
            st = capi.current_stream()
            A.spmv(go["spmv"].view, gi["spmv"].view, st)
            A.spmv(go["spmv_t"].view, gi["spmv_t"].view, st, transposed=True)
            A.spmm(go["spmm2"].view, gi["spmm2"].view, 2, st)
            A.spmm(go["spmm8"].view, gi["spmm8"].view, 8, st)
            A.spmm(go["spmm_t2"].view, gi["spmm_t2"].view, 2, st, transposed=True)
            A.ata(go["ata"].view, gi["ata"].view, tmp.view, st)

        def load(j):
            want = {}
            for name, si, so, k in calls:
                mem.put(gi[name].view, r.run("in", si, j, k))
                mem.fill_bits(go[name].view, LC.PREFILLS["nan"])
                want[name] = r.ata[j] if name == "ata" else r.run("out", so, j, k)
            return want

        def check(want, what):
            s.synchronize()
            for name, si, so, k in calls:
                got = mem.get(go[name].view)
                assert E.bits_equal(got, want[name]), (copy, what, name, E.first_mismatch(got, want[name]))
                assert mem.eq(gi[name].view, mem.const(r.run("in", si, want["j"], k))), (copy, what, name, "input modified")
            for g in list(gi.values()) + list(go.values()) + [tmp]:
                assert g.guards_ok(), (copy, what, g.first_broken())

        want = load(0)
        want["j"] = 0
        launch()
        check(want, "eager")
        g = torch.cuda.CUDAGraph()
        s.synchronize()
        with torch.cuda.graph(g, stream=s):
            launch()
        for j in (1, 2, 1):
            want = load(j)
            want["j"] = j
            g.replay()
            check(want, f"replay with columns {j}..")
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["wide_range", "subnormal_pattern", "wide_range_mid"])
def test_walk_on_three_virtual_ranks(backend, mid, name):
    """fs_dist_spmv / _t / fs_dist_spmm / _t / fs_dist_ata on one matrix across three virtual ranks, vectors in guarded HBM arenas
    and in guarded host arrays, options flipped between the calls (every flip moves the option epoch: the parts are planned again
    for the kernel that runs now), expected bits from tests/_exact.py.  On the mid-size set with panels of 32 rows every rank's
    product is really cut, and the walk opens with products under strict_order (everything with part 0) followed by products under
    the default options: a plan kept from the first would ship rows that the second has not finished"""
    from libfastsparse_amd import capi
    L = backend.L
    big = name == "wide_range_mid"
    d, r = mid if big else (LC.data_sets()[name], LC.refs_of(LC.data_sets()[name]))
    ks = (2,) if big else (2, 4, 5)
    vals = None if d.vals is None else d.vals.ctypes.data
    rng = np.random.default_rng(77)
    devs = (C.c_int * 3)(0, 0, 0)
    D = L.fs_dist_create(3, devs)
    assert D, L.fs_last_error()
    flips = {"reproducible": (0, 1), "strict_order": (0, 1), "spmv_kernel": (0, 1, 7), "spmm_kernel": (0, 1, 3), "cg_fixed_order": (1, 0)}
    log = []
    try:
        # (the mid-size matrix is created under strict_order: the builder does not read it, the parts are planned for the kernel
        # it selects -- everything with part 0 -- and the first product under the default options needs the plan made again)
        with options(binning=2, bin_rows=32 if big else 256, strict_order=int(big)):
            Mx = L.fs_dist_csr_create(D, d.nrow, d.ncol, d.nnz, d.rp.ctypes.data, d.cols.ctypes.data, vals)
            assert Mx, L.fs_last_error()
            assert L.fs_dist_matrix_build_transpose(Mx, d.rp.ctypes.data, d.cols.ctypes.data, vals) == 0, L.fs_last_error()
        n = max(d.nrow, d.ncol)
        vec = {(where, role): LC.Guarded(backend.mem if where == "hbm" else backend.hostmem, f"{role} vector in {where}", n * 5)
               for where in ("hbm", "host") for role in ("in", "out")}
        try:
            with options(**{k: L.fs_get_option(k.encode()) for k in flips}):
                opening = [("spmv",), ("spmv_t",), ("flip", "strict_order", 1), ("spmv",), ("spmv_t",), ("flip", "strict_order", 0), ("spmv",), ("spmv_t",)]
                for step in range(20 if big else 60):
                    forced = opening[step] if step < len(opening) else None
                    op = forced[0] if forced else ("spmv", "spmv_t", "spmm", "spmm_t", "ata", "flip")[int(rng.integers(6))]
                    if op == "flip" or (op == "ata" and not r.ata):
                        k_, vs = list(flips.items())[int(rng.integers(len(flips)))]
                        v = vs[int(rng.integers(len(vs)))]
                        if forced:
                            k_, v = forced[1:]
                        log.append(f"{step} {k_} = {v}")
                        capi.set_option(k_, v)
                        continue
                    side = int(op.endswith("_t"))
                    k = int(rng.choice(ks)) if op.startswith("spmm") else 1
                    where = "host" if k > 1 or rng.integers(2) else "hbm"       # (the k-column entry points take host matrices)
                    wi, wo = (where, "hbm")[int(rng.integers(2))] if k == 1 else "host", where
                    j = int(rng.integers(len(r.ata) if op == "ata" else r.nc - k + 1))
                    gi, go = vec[(wi, "in")], vec[(wo, "out")]
                    xin = r.run("in", side, j, k)
                    want = r.ata[j] if op == "ata" else r.run("out", side, j, k)
                    gi.mem.put(gi.place(xin.size, int(rng.integers(2))), xin)
                    go.mem.fill_bits(go.place(want.size, int(rng.integers(2))), LC.PREFILLS["nan"])
                    log.append(f"{step} {op} k {k} column {j} in {wi} out {wo}")
                    pi, po = gi.mem.ptr(gi.view), go.mem.ptr(go.view)
                    if op == "ata":
                        rc = L.fs_dist_ata(Mx, po, pi, 0.0)
                    elif k == 1:
                        rc = (L.fs_dist_spmv_t if side else L.fs_dist_spmv)(Mx, po, pi)
                    else:
                        rc = (L.fs_dist_spmm_t if side else L.fs_dist_spmm)(Mx, po, pi, k)
                    assert rc == 0, (rc, L.fs_last_error(), log[-12:])
                    got = go.mem.get(go.view)
                    assert E.bits_equal(got, want), (name, E.first_mismatch(got, want), log[-12:])
                    assert gi.mem.eq(gi.view, gi.mem.const(xin)), ("input modified", log[-12:])
                    for g in vec.values():
                        assert g.guards_ok(), (g.first_broken(), log[-12:])
        finally:
            L.fs_dist_matrix_destroy(Mx)
    finally:
        L.fs_dist_destroy(D)


def test_the_poison_probe_saw_poison(backend):
    """last in the file: what poison_heap freed came back to a later allocation with its contents at least once over this module's
    walks -- else the poisoned solves above showed nothing.  (Run alone, the test poisons a few solves of its own first.)"""
    if not POISON["probed"]:
        w = LC.Walk(backend, LC.data_sets()["wide_range_odd"], LC.AUTO, seed=12, steps=0, copies=COPIES)
        with w.session():
            w.create(first=True)
            pair = w.create_pair("exact")
            for i in range(8):
                w.step += 1
                w.exact_solve(pair.A, "pcg", poison=True, pick=i)
        _count_poison(w)
    print(f"poison probes: {POISON['seen']} of {POISON['probed']} doubles still held the poison, {POISON['poisoned']} poisoned solves")
    assert POISON["probed"] > 0 and POISON["seen"] >= 1, POISON
