"""The ORDER of additions of the fixed-order two-pass products (option "reproducible", the solvers' cg_fixed_order), pinned to the
numpy model of tests/_order_model.py on data where almost every reordering changes bits (random 53-bit mantissas x 2^[-8, 8]).

Every copy is forced (binning=2, ldsx=0, tiling=0, long_rows=0) and asserted by name and id form before anything runs on it.
  S   40 000 x 40 000, 3 to 8 entries per row and per column: 3 bands, 4 panels; no two entries of a row in one LDS instruction
  L   20 000 x 30 000, 20 to 60 entries per row: 2 bands; lanes of one instruction hit one slot all the time -- the lane rule
  S8  S with one-byte row ids and no dummy entry: the stream positions are those of the two-byte copy
tests/test_order_model.py holds, on the CPU, that the model differs from the CSR order and from the plain stream order in more
than one row in ten on every one of them: a kernel that added in either of those orders fails here.

LANE_ORDER is the measured rule for two lanes of one ds_add_f64 that hit the same slot (test_model_on_l)."""
import ctypes as C

import numpy as np
import pytest

import _cg_model as CG
import _exact as E
import _large_bands as LB
import _order_model as O
import _pcg_model as P

pytestmark = pytest.mark.gpu

options, _d, _poisoned, _eq = LB.options, LB._d, LB._poisoned, LB._eq
FORCE = dict(binning=2, ldsx=0, tiling=0, long_rows=0)
LANE_ORDER = "ascending"
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"


# ---- copies ----------------------------------------------------------------------------------------------------------
_COPIES = {}


def _create(d, valued, create, sides=2):
    from libfastsparse_amd import capi
    with options(**create):
        A = capi.Matrix.from_csr(d.nrow, d.ncol, _d(d.rp), _d(d.cols), _d(d.vals) if valued else None)
        if sides == 2:
            A.build_transpose(capi.current_stream())
    return A


def _assert_two_pass(A, ids, sides=(0, 1)):
    """two-pass by name; two-byte ids (64) or one-byte ids without a dummy entry (128)"""
    L = LB._lib()
    for t in sides:
        assert A.kernel_name(bool(t)) == "two-pass", (ids, t, A.kernel_name(bool(t)))
        rows8 = L.fs_debug_two_pass_rows8(A.h, t)
        assert rows8 == (0 if ids == 128 else -1), (ids, t, rows8)


def copy_of(shape, ids, valued):
    """the forced two-pass copy of a shape with its A' (ids: bin_flags 64 = two-byte row ids, 128 = one byte), built once"""
    key = (shape, ids, valued)
    if key not in _COPIES:
        A = _create(O.data(shape), valued, dict(bin_flags=ids, **FORCE))
        _assert_two_pass(A, ids)
        _COPIES[key] = A
    return _COPIES[key]


def _plan(shape, t, k=1, order="model", lane_order=LANE_ORDER):
    return O.plan_of(shape, t, k, order, lane_order, LB._ncu(), LB.bin_env())


def _spmv(A, v, n, t, fill=NAN):
    from libfastsparse_amd import capi
    out = _poisoned((n,), fill)
    A.spmv(out, v, capi.current_stream(), transposed=bool(t))
    return out.cpu().numpy()


def _check_geometry(A, shape, t):
    """the device laid out the bands and panels the model assumes"""
    out = (C.c_ulonglong * 8)()
    assert LB._lib().fs_debug_two_pass_layout(A.h, t, out) == 0
    d = O.side(shape, t)
    geo = O.geometry(d, 1, LB._ncu(), LB.bin_env())
    panel, p = O.positions(d, geo)
    B, P = -(-d.ncol // geo["bcols"]), geo["panel_row"].size - 1
    last = np.zeros(P, np.int64)
    np.maximum.at(last, panel, p + 1)
    assert (int(out[6]), int(out[7])) == (B, P), (shape, t, int(out[6]), int(out[7]), B, P)
    assert int(out[5]) == int((-(-last // 16) * 16).sum()), (shape, t, "slots of the stream, paddings included")


def _model_case(A, shape, valued, what, lane_order=LANE_ORDER):
    """A x and A' u under reproducible = 1 are the model's bits and not the CSR order's; strict_order gives the CSR order's"""
    for t in (0, 1):
        d = O.side(shape, t)
        _check_geometry(A, shape, t)
        v = _d(d.x)
        want, csr = _plan(shape, t, lane_order=lane_order)(d.x, valued), _plan(shape, t, order="storage")(d.x, valued)
        with options(reproducible=1):
            assert A.kernel_name(bool(t)) == "two-pass"
            got = _spmv(A, v, d.nrow, t)
        _eq(got, want, (what, "A' u" if t else "A x", "the model's order"))
        assert not E.bits_equal(got, csr), (what, t, "the device adds in CSR order")
        with options(strict_order=1):
            assert A.kernel_name(bool(t)) == "stream"
            _eq(_spmv(A, v, d.nrow, t), csr, (what, t, "strict_order: CSR order"))


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
def test_model_on_s(hip, valued):
    """two-byte ids; no row has two entries in one instruction, so nothing here rests on the lane rule"""
    for t in (0, 1):
        d = O.side("S", t)
        assert O.collisions(d, O.geometry(d, 1, LB._ncu(), LB.bin_env())) == 0
    _model_case(copy_of("S", 64, valued), "S", valued, ("S", valued))


# ---- 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
def test_model_on_s8_captured_first_then_eager(hip, valued):
    """one-byte ids, no dummy: the FIRST fixed-order product of a fresh handle is captured into a graph -- no allocation there, the
    one-wave pass 2 decodes the ids on the fly (the L8 = true instantiation) -- then eager products on the same handle, which
    write the two-byte ids out once and read those"""
    import torch
    from libfastsparse_amd import capi
    d = O.data("S")
    A = _create(d, valued, dict(bin_flags=128, **FORCE))
    _assert_two_pass(A, 128)
    xd, y = _d(d.x), _poisoned((d.nrow,), NAN)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with options(reproducible=1):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            A.spmv(y, xd, capi.current_stream())
        g.replay()
        torch.cuda.synchronize()
    _eq(y.cpu().numpy(), _plan("S", 0)(d.x, valued), ("S8", valued, "captured first fixed-order product"))
    del g
    _model_case(A, "S", valued, ("S8", valued, "eager"))
    A.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
def test_model_on_l(hip, valued):
    """Rows of 20 to 60 entries: 732 248 (A) and 618 691 (A') pairs of entries of one row sit in one LDS instruction.  Measured on
    an MI355X: the LDS adds the lanes of one ds_add_f64 that hit the same slot in ASCENDING lane order -- that single rule
    explains every row of A x and A' u, valued and pattern-only, and the descending rule differs in 38 to 63 % of the rows."""
    A = copy_of("L", 64, valued)
    other = "descending" if LANE_ORDER == "ascending" else "ascending"
    with options(reproducible=1):
        for t in (0, 1):
            d = O.side("L", t)
            got = _spmv(A, _d(d.x), d.nrow, t)
            for rule in (LANE_ORDER, other):
                want = _plan("L", t, lane_order=rule)(d.x, valued)
                print(f"L {'At' if t else 'A'} {'valued' if valued else 'pattern'} lanes {rule}: "
                      f"{int((got.view(np.int64) != want.view(np.int64)).sum())} of {got.size} rows differ from the model")
    _model_case(A, "L", valued, ("L", valued))


# ---- 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
@pytest.mark.parametrize("shape", ["S", "L"])
def test_k_columns(hip, shape, valued):
    """k = 2 and 4 on the k-column copies (bands of 8 192 / 4 096 columns, 4 / 2 entries per lane): every column of A X and A' U
    has the bits of the k-column model under the lane rule of test_model_on_l, and not those of the CSR order"""
    from libfastsparse_amd import capi
    A = copy_of(shape, 64, valued)
    st = capi.current_stream()
    for k in (2, 4):
        for t in (0, 1):
            with options(**FORCE):
                A.prepare(k, st, transposed=bool(t))
            assert A.spmm_plan(k, bool(t)) == "k-column two-pass", (shape, k, t, A.spmm_plan(k, bool(t)))
            d = O.side(shape, t)
            X = d.X(k)
            want, csr = _plan(shape, t, k)(X, valued), _plan(shape, t, k, "storage")(X, valued)
            with options(reproducible=1):
                assert A.spmm_plan(k, bool(t)) == "k-column two-pass"
                Y = _poisoned((d.nrow, k), NAN)
                A.spmm(Y, _d(X), k, st, transposed=bool(t))
            got = Y.cpu().numpy()
            for j in range(k):
                _eq(got[:, j], want[:, j], (shape, valued, k, t, "column", j))
            assert not E.bits_equal(got, csr), (shape, valued, k, t, "the device adds in CSR order")


# ---- 5 ---------------------------------------------------------------------------------------------------------------
def _one_answer(A, d, sides, rebuild, what, valued=True, strided_k=3, strided_plans=(LB.BINNED_COLS,), want=None):
    """under reproducible = 1 every way of launching the product on a side gives the bits of the whole product (`want`, or the first
    whole product): in 3 and 4 parts, host vectors, a graph replay, strided x and y, a second handle from the same arrays, the handle
    without its plain CSR and with it again, and 5 products issued while a second stream keeps the GPU busy"""
    import torch
    from libfastsparse_amd import capi
    L = LB._lib()
    st = capi.current_stream()
    dt = O.transposed(d) if 1 in sides else None
    A2 = rebuild()
    with options(reproducible=1):
        for t in sides:
            dd = dt if t else d
            v, n = _d(dd.x), dd.nrow
            whole = _spmv(A, v, n, t)
            if want is not None:
                _eq(whole, want[t], (what, t, "the whole product"))
            _eq(_spmv(A, v, n, t, -0.0), whole, (what, t, "run to run"))
            for nparts in (3, 4):
                y = _poisoned((n,), NAN)
                for p in range(nparts):
                    A.spmv_part(y, v, p, nparts, st, transposed=bool(t))
                _eq(y.cpu().numpy(), whole, (what, t, "in", nparts, "parts"))
            yh = np.full(n, np.nan)
            A.spmv_host(yh, dd.x, transposed=bool(t))
            _eq(yh, whole, (what, t, "host vectors"))
            # a graph replay
            y = _poisoned((n,), NAN)
            torch.cuda.synchronize()
            s = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                A.spmv(y, v, capi.current_stream(), transposed=bool(t))
            y.fill_(NAN)
            g.replay()
            torch.cuda.synchronize()
            _eq(y.cpu().numpy(), whole, (what, t, "graph replay"))
            del g
            # strided x and y: column 0 is x
            k = strided_k
            with options(**({"spmm_kernel": 3} if k == 3 else {})):
                assert L.fs_matrix_spmm_plan(A.h, k, t) in strided_plans, (what, t, L.fs_matrix_spmm_plan(A.h, k, t))
                X = dd.X(k)
                Y = _poisoned((n, k), NAN)
                A.spmm(Y, _d(X), k, st, transposed=bool(t))
                Y = Y.cpu().numpy()
            _eq(Y[:, 0], whole, (what, t, "strided, column 0"))
            _eq(Y[:, k - 1], _spmv(A, _d(X[:, k - 1]), n, t), (what, t, "strided, last column against its own product"))
            # a second handle built from the same arrays
            _eq(_spmv(A2, v, n, t), whole, (what, t, "a second handle"))
            # while a second stream keeps the GPU busy with unrelated work
            side_stream = torch.cuda.Stream()
            m = torch.ones((1024, 1024), dtype=torch.float32, device="cuda")
            ys = [_poisoned((n,), NAN) for _ in range(5)]
            torch.cuda.synchronize()
            for y in ys:
                with torch.cuda.stream(side_stream):
                    for _ in range(4):
                        m = (m @ m) * (1.0 / 1024)
                A.spmv(y, v, st, transposed=bool(t))
            torch.cuda.synchronize()
            for i, y in enumerate(ys):
                _eq(y.cpu().numpy(), whole, (what, t, "beside a busy stream, product", i))
        # without the plain CSR arrays, and with them again
        wholes = {t: _spmv(A2, _d((dt if t else d).x), (dt if t else d).nrow, t) for t in sides}
        assert A2.release_csr() >= 1, (what, "nothing released")
        for t in sides:
            dd = dt if t else d
            _eq(_spmv(A2, _d(dd.x), dd.nrow, t), wholes[t], (what, t, "after release_csr"))
        for t in sides:
            dd = dt if t else d
            A2.restore_csr(_d(dd.rp), _d(dd.cols), _d(dd.vals) if valued else None, transposed=bool(t))
        for t in sides:
            dd = dt if t else d
            _eq(_spmv(A2, _d(dd.x), dd.nrow, t), wholes[t], (what, t, "after restore_csr"))
    A2.close()


@pytest.mark.parametrize("valued", [True, False], ids=["valued", "pattern"])
@pytest.mark.parametrize("shape", ["S", "L"])
def test_one_product_one_answer(hip, shape, valued):
    """S and L on the two-byte two-pass copy: every launch form carries the model's bits"""
    A = copy_of(shape, 64, valued)
    d = O.data(shape)

    def rebuild():
        A2 = _create(d, valued, dict(bin_flags=64, **FORCE))
        _assert_two_pass(A2, 64)
        return A2

    want = {t: _plan(shape, t)(O.side(shape, t).x, valued) for t in (0, 1)}
    _one_answer(A, d, (0, 1), rebuild, (shape, valued), valued, want=want)


def test_one_product_one_answer_long_rows(hip):
    """a forced long-row copy (rows of >= 32 entries out of the two-pass copy: the segmented scan, ypart and the combine pass, of
    which there is no model): only the invariance.  The 150 000 x 200 000 heavy-tailed pattern of test_long_rows_are_exact with
    values that round."""
    L = LB._lib()
    h = LB.heavy()
    d = O.round_data("heavy", h.nrow, h.ncol, h.rows, h.cols, 61)
    create = dict(binning=2, long_rows=2, long_min_len=32)

    def rebuild():
        A2 = _create(d, True, create, sides=1)
        info = (C.c_int64 * 2)()
        assert A2.kernel_name() == "two-pass" and L.fs_debug_long_rows(A2.h, 0, info) == 0 and info[0] > 0, info[0]
        return A2

    A = rebuild()
    _one_answer(A, d, (0,), rebuild, "long rows")
    A.close()


def test_one_product_one_answer_lds_staged(hip):
    """a forced LDS-staged copy that can be ordered (every row of a work item with one wave, chunks of a panel adding in turn: no
    model either): only the invariance; no chunk gave up waiting for its turn.  Strided: k = 2, the strided sweeps of that kernel."""
    L = LB._lib()
    L.fs_debug_ldsx_orderable.argtypes = [C.c_void_p, C.c_int]
    L.fs_debug_ldsx_ticket_giveups.argtypes = [C.c_void_p, C.c_int]
    d = O.data("L")
    create = dict(ldsx=2, binning=0, tiling=0)

    def rebuild():
        A2 = _create(d, True, create)
        for t in (0, 1):
            assert A2.kernel_name(bool(t)) == "lds-staged" and L.fs_debug_ldsx_orderable(A2.h, t) == 1, (t, A2.kernel_name(bool(t)))
        return A2

    A = rebuild()
    with options(reproducible=1):
        assert A.kernel_name() == "lds-staged" and A.kernel_name(True) == "lds-staged"
    _one_answer(A, d, (0, 1), rebuild, "lds-staged", strided_k=2, strided_plans=(6,))
    for t in (0, 1):
        assert L.fs_debug_ldsx_ticket_giveups(A.h, t) == 0, t
    A.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------
SYSTEMS = CG.systems(large=False)


@pytest.mark.parametrize("name", ["valued", "binary_F257"])
def test_solvers_in_their_default_mode_are_the_model(hip, name):
    """fs_cg and fs_pcg (Jacobi) with cg_fixed_order at its default and strict_order off, on the two-byte two-pass pair: x, the
    iteration count and the final st[] are the solver models' with A p and A' y taken from the order model"""
    import torch
    from libfastsparse_amd import capi
    L = LB._lib()
    L.fs_debug_last_cg_state.argtypes = [C.c_void_p]
    L.fs_debug_fixed_order_honoured.argtypes = [C.c_void_p, C.c_int]
    s = SYSTEMS[name]
    assert L.fs_get_option(b"cg_fixed_order") == 1 and L.fs_get_option(b"strict_order") == 0
    vals = None if s.vals is None else _d(s.vals)
    with options(bin_flags=64, **FORCE):
        A = capi.Matrix.from_coo(s.nrow, s.ncol, _d(s.rows), _d(s.cols), vals)
        At = capi.Matrix.from_coo(s.ncol, s.nrow, _d(s.cols), _d(s.rows), vals)
    for M_ in (A, At):
        _assert_two_pass(M_, 64, sides=(0,))
        assert L.fs_debug_fixed_order_honoured(M_.h, 0) == 1
    t_csr = s.t_csr_coo()
    da, dt = O.from_csr("A", s.nrow, s.ncol, s.a_csr()), O.from_csr("At", s.ncol, s.nrow, t_csr)
    pa, pt = (O.Plan(m, O.geometry(m, 1, LB._ncu(), LB.bin_env()), "model", LANE_ORDER) for m in (da, dt))
    amul, atmul = (lambda p: pa(p)), (lambda y: pt(y))
    st = capi.current_stream()

    def state():
        raw = np.full(CG.CG_STATE_DOUBLES, np.nan)
        assert L.fs_debug_last_cg_state(raw.ctypes.data) == CG.CG_STATE_DOUBLES
        return raw

    # the products of the solve are the model's (and the storage-order model of the strict tests is another function on this system)
    with options(reproducible=1):
        _eq(_spmv(A, _d(s.b), s.nrow, 0), amul(s.b), (name, "A b"))
        _eq(_spmv(At, _d(amul(s.b)), s.ncol, 0), atmul(amul(s.b)), (name, "A' (A b)"))
    model = CG.cg(s.ncol, amul, atmul, s.b, s.lam, s.tol)
    x = torch.full((s.ncol,), NAN, dtype=torch.float64, device="cuda")
    it = C.c_int(-1)
    capi.check(L.fs_cg(A.h, At.h, x.data_ptr(), _d(s.b).data_ptr(), s.lam, s.tol, C.byref(it), st), "fs_cg")
    bad = CG.mismatch(x.cpu().numpy(), model.x, it.value, model.iterations, CG.state_from_device(state(), False), model.state)
    assert bad is None, f"fs_cg on {name}: {bad}"
    assert model.iterations >= 5, (name, model.iterations)

    pm = P.pcg(s.ncol, amul, atmul, s.b, s.lam, s.tol, 0, P.dinv_of(P.gram_diag(t_csr, s.lam)))
    x = torch.full((s.ncol,), NAN, dtype=torch.float64, device="cuda")
    info = capi.pcg(A, At, x, _d(s.b), s.lam, s.tol, max_iter=0, precond=P.PRECOND_JACOBI, warm_start=False, diag=None, stream=st)
    bad = CG.mismatch(x.cpu().numpy(), pm.x, info.iterations, pm.iterations, P.state_from_device(state()), pm.state)
    assert bad is None, f"fs_pcg (Jacobi) on {name}: {bad}"
    A.close()
    At.close()
