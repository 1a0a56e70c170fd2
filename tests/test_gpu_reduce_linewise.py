"""Pass 2 of the two-pass SpMV, which reads its stream line-wise (a lane owns the entry pairs {2 l, 2 l + 1} of four 128-entry
blocks per step), with its product loads non-temporal (the default) and plain (bin_flags 256 at product time), through the public
product only.

The shapes are the smallest at which the decode of a form can go wrong: a stream shorter than one round of 16 384 entries, a
stream of whole rounds and the same plus one group of 16, several panels and bands with whole and partial rounds, row steps above
255 (dummy entries of the one-byte ids), and copies forced to two-byte and to one-byte ids.

Integer-valued data are exactly summable, so both policies must give the same bits, those of the exact sums; on other data a product stays within 1e-12 x row length of the strict_order product (|a|, |x| <= 1)."""
import ctypes as C

import numpy as np
import pytest

from _gpu import options as _options, to_device as _d

pytestmark = pytest.mark.gpu

ROUND = 16384
PLAIN = 256
FLAGS = [PLAIN]
IDS = {"two-byte": 64, "one-byte": 128}


def _csr(nrow, ncol, lengths, seed):
    """CSR with the given row lengths, ascending columns in every row"""
    rng = np.random.default_rng(seed)
    rp = np.zeros(nrow + 1, np.int32)
    np.cumsum(lengths, out=rp[1:])
    cols = np.empty(int(rp[-1]), np.int32)
    for r in np.flatnonzero(lengths):
        cols[rp[r]:rp[r + 1]] = np.sort(rng.choice(ncol, int(lengths[r]), replace=False))
    return rp, cols


def _uniform(nrow, ncol, per, seed):
    """`per` entries in every row, one in each of `per` equal strides of the columns"""
    rng = np.random.default_rng(seed)
    rp = np.arange(nrow + 1, dtype=np.int32) * per
    stride = ncol // per
    cols = (np.arange(per, dtype=np.int32) * stride + rng.integers(0, stride, (nrow, per), dtype=np.int32)).reshape(-1)
    return rp, cols


def _short():
    return (500, 700) + _uniform(500, 700, 8, 1)                       # 4000 entries: no whole round


def _whole_rounds():
    return (2048, 3000) + _uniform(2048, 3000, 16, 2)                  # one cell of 32 768 entries: two rounds, nothing left


def _whole_rounds_plus_group():
    lengths = np.full(2048, 16)
    lengths[1000] = 17                                                 # 32 769 entries: padded to two rounds and one group
    return (2048, 3000) + _csr(2048, 3000, lengths, 3)


def _panels_and_bands():
    return (40000, 40000) + _uniform(40000, 40000, 16, 4)              # 3 panels x 3 bands, 213 K entries a panel


def _row_gaps():
    # rows 300 or 700 apart inside a cell: every step is walked by one or two dummy entries of the one-byte ids
    nrow, ncol = 30000, 20000
    lengths = np.zeros(nrow, np.int64)
    lengths[np.cumsum(np.tile([300, 700, 300], 20))] = 40
    lengths[5:45] = 3                                                  # and a stretch of neighbouring rows
    return (nrow, ncol) + _csr(nrow, ncol, lengths, 5)


SHAPES = {"short": _short, "whole rounds": _whole_rounds, "whole rounds + group": _whole_rounds_plus_group,
          "panels and bands": _panels_and_bands, "row gaps": _row_gaps}
# padded stream length of the single-cell shapes (checked against the copy: the shapes are what the names say)
STREAM = {"short": 4000, "whole rounds": 2 * ROUND, "whole rounds + group": 2 * ROUND + 16}


def _layout(A, transposed):
    from libfastsparse_amd import capi
    L = capi.lib()
    out = (C.c_ulonglong * 8)()
    L.fs_debug_two_pass_layout.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]
    assert L.fs_debug_two_pass_layout(A.h, int(transposed), out) == 0
    L.fs_debug_two_pass_rows8.restype = C.c_longlong
    L.fs_debug_two_pass_rows8.argtypes = [C.c_void_p, C.c_int]
    return int(out[5]), int(L.fs_debug_two_pass_rows8(A.h, int(transposed)))


def _exact_sums(nrow, rp, cols, vals, x):
    t = x[cols] if vals is None else vals * x[cols]
    return np.add.reduceat(np.append(t, 0.0), rp[:-1])[:nrow] * (np.diff(rp) > 0)


@pytest.fixture(scope="module", params=list(SHAPES))
def shape(request):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    nrow, ncol, rp, cols = SHAPES[request.param]()
    rng = np.random.default_rng(99)
    data = dict(name=request.param, nrow=nrow, ncol=ncol, rp=rp, cols=cols, rows=np.repeat(np.arange(nrow, dtype=np.int32), np.diff(rp)),
                vals_int=rng.integers(-8, 9, cols.size).astype(np.float64), vals_real=rng.uniform(-1.0, 1.0, cols.size),
                x_int=rng.integers(-1000, 1001, ncol).astype(np.float64), x_real=np.sin(7.0 * np.arange(ncol) + 0.3),
                u_int=rng.integers(-1000, 1001, nrow).astype(np.float64), u_real=np.sin(11.0 * np.arange(nrow) - 0.2))
    return data


def _matrix(d, ids, vals):
    from libfastsparse_amd import capi
    with _options(binning=2, ldsx=0, tiling=0, long_rows=0, bin_flags=IDS[ids]):
        A = capi.Matrix.from_csr(d["nrow"], d["ncol"], _d(d["rp"]), _d(d["cols"]), None if vals is None else _d(vals))
        A.build_transpose(capi.current_stream())
    for tr in (False, True):
        assert A.kernel_name(tr) == "two-pass", (d["name"], ids, tr, A.kernel_name(tr))
        n, dummies = _layout(A, tr)
        assert (dummies >= 0) == (ids == "one-byte"), (d["name"], ids, tr, dummies)
        if not tr and d["name"] in STREAM:
            assert n == (STREAM[d["name"]] + 15) // 16 * 16 and dummies <= 0, (d["name"], n, dummies)
        if not tr and d["name"] == "row gaps" and ids == "one-byte":
            assert dummies >= 59, dummies
    return A


def _product(A, v, n, flags, transposed, **mode):
    import torch
    from libfastsparse_amd import capi
    out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    with _options(bin_flags=flags, **mode):
        A.spmv(out, v, capi.current_stream(), transposed=transposed)
    return out.cpu().numpy()


@pytest.mark.parametrize("valued", [False, True], ids=["pattern", "valued"])
@pytest.mark.parametrize("ids", list(IDS))
def test_load_policies_keep_the_bits_on_integer_data(shape, ids, valued):
    """A x and A' u under both load policies: the same bits, which are the exact sums"""
    d = shape
    vals = d["vals_int"] if valued else None
    A = _matrix(d, ids, vals)
    x, u = _d(d["x_int"]), _d(d["u_int"])
    want_y = _exact_sums(d["nrow"], d["rp"], d["cols"], vals, d["x_int"])
    t = d["u_int"][d["rows"]] if vals is None else vals * d["u_int"][d["rows"]]
    want_z = np.zeros(d["ncol"])
    np.add.at(want_z, d["cols"], t)
    base_y, base_z = _product(A, x, d["nrow"], 0, False), _product(A, u, d["ncol"], 0, True)
    assert np.array_equal(base_y, want_y) and np.array_equal(base_z, want_z), (d["name"], ids, "default path")
    for flags in FLAGS:
        y, z = _product(A, x, d["nrow"], flags, False), _product(A, u, d["ncol"], flags, True)
        assert y.tobytes() == base_y.tobytes(), (d["name"], ids, flags, "A x", np.flatnonzero(y != base_y)[:8])
        assert z.tobytes() == base_z.tobytes(), (d["name"], ids, flags, "A' u", np.flatnonzero(z != base_z)[:8])
    A.close()


@pytest.mark.parametrize("valued", [False, True], ids=["pattern", "valued"])
@pytest.mark.parametrize("ids", list(IDS))
def test_load_policies_stay_within_the_rounding_bound(shape, ids, valued):
    """the same on data that round: within 1e-12 x row length of the strict_order product (|a|, |x| <= 1)"""
    d = shape
    A = _matrix(d, ids, d["vals_real"] if valued else None)
    x, u = _d(d["x_real"]), _d(d["u_real"])
    ref_y, ref_z = _product(A, x, d["nrow"], 0, False, strict_order=1), _product(A, u, d["ncol"], 0, True, strict_order=1)
    len_y, len_z = np.diff(d["rp"]), np.bincount(d["cols"], minlength=d["ncol"])
    for flags in [0] + FLAGS:
        y, z = _product(A, x, d["nrow"], flags, False), _product(A, u, d["ncol"], flags, True)
        assert np.all(np.abs(y - ref_y) <= 1e-12 * len_y), (d["name"], ids, flags, "A x", float(np.max(np.abs(y - ref_y))))
        assert np.all(np.abs(z - ref_z) <= 1e-12 * len_z), (d["name"], ids, flags, "A' u", float(np.max(np.abs(z - ref_z))))
    A.close()
