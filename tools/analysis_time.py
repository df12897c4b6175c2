"""Cost of the structure analysis at C3 (1e6 proteins) after 2000 steps, against
kmc_get_clusters — the only comparable capability before it.  Run by hand:
  python tools/analysis_time.py [--workload C3] [--steps 2000] [--repeats 20] [--out profiles/analysis_C3.json]
For each of census (8 x 4 bins), pair_counts (AA, r_max 300, 60 bins) and
get_clusters: the median and minimum wall time of a call over the repeats
(what the caller waits for: launches, the wait, the result copies), and for
the two device analyses the HIP-event time of the call's kernels
(kmc_analysis_ms).  kmc_get_clusters launches nothing: it is copies and a host
loop, so wall time is its only measure."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = "kmc-with-a-diffusion-reaction-algorithm_amd"
engine = importlib.import_module(PKG + ".engine")
workloads = importlib.import_module(PKG + ".workloads")

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="C3")
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--out", default=None)
a = ap.parse_args()

p = workloads.params(a.workload)
res = {"workload": a.workload, "n_a": p.n_a, "n_b": p.n_b, "steps": a.steps, "repeats": a.repeats}
with engine.Simulation(p) as sim:
    sim.init_random()
    done = 0
    while done < a.steps:
        n = min(500, a.steps - done)
        sim.step(n)
        done += n

    def timed(name, f, device):
        f()  # warm: the first call allocates the scratch
        wall, dev = [], []
        for _ in range(a.repeats):
            t = time.perf_counter()
            f()
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(sim.analysis_ms)
        res[name] = {"wall_ms_median": statistics.median(wall), "wall_ms_min": min(wall)}
        if device:
            res[name].update(device_ms_median=statistics.median(dev), device_ms_min=min(dev))

    timed("census", lambda: sim.census(8, 4), True)
    timed("pair_counts_AA_300", lambda: sim.pair_counts("AA", 300.0, 60), True)
    timed("get_clusters", sim.clusters, False)
    _, c = sim.census(8, 4)
    res["census_summary"] = c.as_dict()
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
