#!/usr/bin/env python3
"""Randomised differential run of every CG solver after fs_cg2 (fs_pcg, fs_mscg, fs_pcgn, fs_pcgn_lambdas, fs_mscgn and their
fs_dist_* forms on 1, 3 or 5 virtual ranks) against a reference that shares no code with the models: a dense solve of
(A'A + lambda I) x = b in numpy.longdouble and a textbook preconditioned CG (tests/_truth.py, where the draw, the checks and the
origin of every bar are written down).  Every draw is solved to F twice and once with a cap by every solver, and the relations the
header states between solvers are checked bit for bit.  One process; the first failing check ends the run with the draw's seed and
number, and `--cases N:N+1` with the same seed replays exactly that draw; nothing is retried.

    python tools/fuzz_solvers.py [seconds] [seed] [--solver NAME] [--cases N | --cases FIRST:END]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

import _fuzz_solvers as FZ  # noqa: E402
import _gpu  # noqa: E402
import _truth as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("seconds", nargs="?", type=float, default=120.0)
ap.add_argument("seed", nargs="?", type=int, default=99)
ap.add_argument("--solver", choices=T.SOLVERS, default=None, help="one solver only (and no relations)")
ap.add_argument("--cases", default=None, help="N: draws 0 .. N - 1 whatever the time; FIRST:END: those draws")
args = ap.parse_args()
first, end = 0, None
if args.cases:
    first, end = (int(v) for v in args.cases.split(":")) if ":" in args.cases else (0, int(args.cases))
L = _gpu.gpu_lib()
solvers = (args.solver,) if args.solver else T.SOLVERS
tallies = {s: T.Tally() for s in solvers}
t_end = time.time() + args.seconds
draw, compared = first, 0
while (draw < end) if end is not None else (time.time() < t_end):
    case = T.make_case(np.random.default_rng([args.seed, draw]), args.seed, draw)
    try:
        for s in solvers:
            tallies[s].add(case, s, FZ.run_and_check(L, case, s))
        if not args.solver:
            compared += FZ.relations(L, case)
    except T.CheckFailed as e:
        print(f"fuzz_solvers: FAILED at seed {args.seed} draw {draw} (replay: --cases {draw}:{draw + 1}): {e}", flush=True)
        sys.exit(1)
    draw += 1
    if (draw - first) % 10 == 0:
        print(f"{draw - first} draws ok", flush=True)
for s in solvers:
    assert tallies[s].cases < 20 or tallies[s].share() >= T.CLASS_FLOOR, tallies[s].line(s)
print(f"fuzz_solvers: {draw - first} draws (seed {args.seed}, draws {first} .. {draw - 1}), all within the bars; {compared} pairs of solves "
      f"compared bit for bit for the header's relations; " + "; ".join(tallies[s].line(s) for s in solvers))
