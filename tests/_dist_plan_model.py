"""A numpy restatement of the exchange layout of the sharded products (libfastsparse_amd/csrc/fs_dist_plan.h).

Integers in, integers out, in the order of the C++: tests/test_dist_plan.py compares the two element for element on the CPU.
bounds: n + 1 row bounds of the ranks; cut: (n, np + 1) row cuts of every rank's local product; k: columns.
"""
import numpy as np


def most_busy_parts(cut):
    cut = np.asarray(cut, np.int64).reshape(len(cut), -1)
    return int((np.diff(cut, axis=1) > 0).sum(axis=1).max()) if cut.size else 0


def plan_exchange(n, k, bounds, cut):
    bounds = np.asarray(bounds, np.int64)
    cut = np.asarray(cut, np.int64).reshape(n, -1)
    np_ = cut.shape[1] - 1
    rows = np.diff(cut, axis=1)                                   # [rank][part]
    shard = np.diff(bounds)
    max_rows = int(shard.max())
    maxc = rows.max(axis=0) if np_ else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum(n * maxc)]).astype(np.int64)
    # the overlapped layout: part after part, rank after rank, parts without rows left out
    p, r = np.meshgrid(np.arange(np_), np.arange(n), indexing="ij")
    p, r = p.ravel(), r.ravel()
    keep = rows[r, p] > 0
    p, r = p[keep], r[keep]
    dst = (bounds[r] + cut[r, p]) * k
    src = (off[p] + r * maxc[p]) * k
    cnt = rows[r, p] * k
    # the whole-shard layout: rank r's rows at r * max_rows
    own = np.nonzero(shard > 0)[0]
    table = np.concatenate([dst, src, cnt, bounds[own] * k, own * max_rows * k, shard[own] * k]).astype(np.int64)
    return {
        "scalars": [n, k, np_, int(most_busy_parts(cut) > 1), max_rows, len(cnt), len(own), int(cnt.max()) if len(cnt) else 0,
                    max(int(off[-1]), n * max_rows), 2 * max_rows + 1, max_rows, most_busy_parts(cut), 3 * len(cnt)],
        "maxc": [int(v) for v in maxc],
        "off": [int(v) for v in off],
        "table": [int(v) for v in table],
        "cut": [int(v) for v in cut.ravel()],
    }
