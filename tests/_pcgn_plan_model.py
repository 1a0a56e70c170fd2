"""A numpy restatement of the narrowing schedule of fs_pcgn / fs_pcgn_lambdas under option "pcgn_compact", written from the text of
include/fastsparse_hip.h (fs_pcgn, "Narrowing"), not from libfastsparse_amd/csrc/fs_pcgn_plan.h: tests/test_pcgn_plan.py compares the
two on the CPU, tests/test_gpu_pcgn_compact.py compares a solve's own segments with this.

counts[j]: column j's final count; frozen0[j]: frozen by the start kernels; cap: the iteration cap; usable: the rungs below k the
solve may narrow to.  Segments are (first iteration, width, mask of original columns)."""
import numpy as np

RUNGS = (1, 2, 4, 8, 16, 32)


def rung(L):
    """W(L): the smallest rung that holds L columns"""
    return min(w for w in RUNGS if w >= L)


def all_columns(k):
    return (1 << k) - 1


def usable_bits(widths):
    return sum(set(widths))


def plan(k, usable, counts, frozen0, cap):
    counts = np.asarray(counts, np.int64)
    start = ~np.asarray(frozen0, bool)
    segments = [(0, k, all_columns(k))]
    if not start.any():
        return segments                                           # done before the first iteration
    # iteration i runs iff a column is live after iteration i - 1; the last one is that of the longest column, or cap - 1
    last = int(np.minimum(counts[start], cap - 1).max())
    width = k
    for n in range(last + 1):
        live = start if n < 2 else start & (counts > n - 2)       # what the host knows: the mask after iteration n - 2
        fits = [w for w in usable if rung(int(live.sum())) <= w < width]
        if not fits:
            continue
        width = min(fits)
        seg = (n, width, int(sum(1 << int(j) for j in np.nonzero(live)[0])))
        if segments[-1][0] == n:
            segments[-1] = seg
        else:
            segments.append(seg)
    return segments


def of_solve(k, usable, infos, cs, cap):
    """the plan of a solve from its own outcome: the infos and the per-column scalars by name"""
    counts = [i.iterations for i in infos]
    frozen0 = [i.iterations == 0 and i.converged == 1 and c["rz"] == 0.0 and c["alpha"] == 0.0 for i, c in zip(infos, cs)]
    return plan(k, usable, counts, frozen0, cap)
