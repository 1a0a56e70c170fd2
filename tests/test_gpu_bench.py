"""`bench.py` on one GPU, as the driver runs it (a short config-2 run): the line's contract keys, and roofline.traffic MEASURED by the
run itself -- two rocprofv3 --pmc children after the timed region (bench.live_pmc_traffic) -- next to the value of profiles/."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_measures_its_own_hbm_traffic():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c2", "--steps", "5", "--warmup", "1", "--full",
                        "--no-cpu-baseline", "--no-reproducible-cost"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    rec = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline"):
        assert key in rec, key
    assert rec["n_gpus"] == 1 and rec["steps"] == 5 and rec["dtype"] == "f64" and rec["vs_baseline"] is None
    r = rec["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    if "traffic_live_measurement_failed" in r:      # the profiler itself could not run here (no counters for this user, a time-out): not the product's fault
        assert r["traffic"] and r["traffic_from_profiles"]["measured_by_this_run"] is False      # the line then says so and keeps the value of profiles/
        pytest.skip("rocprofv3 --pmc did not run on this box: %r" % (r["traffic_live_measurement_failed"],))
    m = r["traffic_measured"]
    assert m["measured_by_this_run"] is True and set(m["bytes_per_kernel"]) == {"fs::spmv_expand_kernel", "fs::spmv_reduce_"}
    assert abs(sum(m["bytes_per_kernel"].values()) - r["traffic"]) < 1.0
    alg = r["algorithmic_bytes_per_launch"]
    # the two-pass pair moves 28.25 B per entry for 12 algorithmic ones: between 2 x and 2.6 x, and close to what profiles/ holds
    assert 2.0 * alg < r["traffic"] < 2.6 * alg, (r["traffic"], alg)
    old = r["traffic_from_profiles_for_comparison"]["traffic"]
    assert old and abs(r["traffic"] - old) < 0.03 * old, (r["traffic"], old)
    assert 0.2 < r["frac"] < r["design_ceiling_frac"] < 0.45
    # a third child under `rocprofv3 --kernel-trace` alone: the tracer's clock on the product's kernels against the HIP-event pair of
    # the SAME process (kernels run a few percent slower under the tracer than in the untraced parent, hence two ratios)
    assert 0.97 < r["hip_events_over_kernel_trace_same_process"] < 1.05, r
    assert 0.85 < r["hip_events_over_kernel_trace"] < 1.10, r


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """a plain run (no --full): the timed steps and a short headline only, and --dump-outputs writes the y = A x and z = A' u of
    the last timed step -- checked against the oracle's products of the same generated matrix"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from oracle import pyoracle as O
    from oracle import pysynth
    n, per = 200_000, 16
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--rows", str(n),
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 4096, p.stdout[-2000:]
    rec = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert key in rec, key
    assert rec["steps"] == 4 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["dtype"] == "f64"
    assert "also" not in rec and "cpu_baseline" not in rec and "self_check" not in rec["config"]
    assert sorted(os.listdir(out)) == ["y.npy", "z.npy"]
    y, z = np.load(out / "y.npy"), np.load(out / "z.npy")
    assert y.dtype == np.float64 and z.dtype == np.float64 and y.shape == (n,) and z.shape == (n,)
    rp, cc, vv = pysynth.uniform(n, n, per, bench.SEED_C2)
    x = np.sin(7.0 * np.arange(n, dtype=np.float64) + 0.3)
    u = np.sin(11.0 * np.arange(n, dtype=np.float64) - 0.2)
    scale = O.csr_abs_scale(n, rp, cc, vv, x)
    assert np.all(np.abs(y - O.csr_mul(n, rp, cc, vv, x)) <= 1e-12 * scale)
    rows = np.repeat(np.arange(n, dtype=np.int32), per)
    zscale = O.coo_tmul(n, rows, cc, np.abs(vv), np.abs(u))
    assert np.all(np.abs(z - O.coo_tmul(n, rows, cc, vv, u)) <= 1e-12 * zscale)


def test_dump_sample_is_fixed_and_within_budget():
    """--dump-outputs keeps at most 48 MB: a larger vector is written as the same seeded, ascending sample in every run"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    a, b = bench.sample_index(10_000_000, 1000), bench.sample_index(10_000_000, 1000)
    assert np.array_equal(a, b) and len(np.unique(a)) == 1000 and np.all(np.diff(a) > 0) and a[-1] < 10_000_000
    assert bench.DUMP_BYTES <= 64 << 20
