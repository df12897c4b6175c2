"""Cost of the cluster geometry at C3 (1e6 proteins) after 2000 steps, beside the
oligomer census and against the route a user had before it: get_state() plus a
sequential unwrap on the host (kmc_host_cluster_geometry).  Run by hand:
  python tools/geometry_time.py [--workload C3] [--steps 2000] [--repeats 20] [--out profiles/geometry_C3.json]
For each of cluster_geometry (64 bins), cluster_list (min_size 4), unwrap and
census (8 x 4 bins): the median and minimum wall time of a call over the
repeats (what the caller waits for: launches, the wait, the result copies) and
the HIP-event time of the call's kernels (kmc_analysis_ms).  get_state and the
host walk launch nothing the events could see: wall time is their only measure.
The device table is compared with the host's at this size before it is timed."""
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
ap.add_argument("--max-size", type=int, default=64)
ap.add_argument("--out", default=None)
a = ap.parse_args()

p = workloads.params(a.workload)
res = {"workload": a.workload, "n_a": p.n_a, "n_b": p.n_b, "steps": a.steps, "repeats": a.repeats,
       "max_size": a.max_size}
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

    hs = sim.get_state()
    table, out = sim.cluster_geometry(a.max_size)
    h = engine.host_cluster_geometry(p, hs, a.max_size)
    label, shift, span = sim.unwrap()
    same = (table.tobytes() == h[3].tobytes() and out.as_dict() == h[4].as_dict() and (label == h[0]).all()
            and (shift == h[1]).all() and (span == h[2]).all())
    res["device_equals_host"] = bool(same)
    if not same:
        raise SystemExit("geometry_time: the device and the host results differ at this size")

    timed("cluster_geometry", lambda: sim.cluster_geometry(a.max_size), True)
    timed("cluster_list_4", lambda: sim.cluster_list(4, cap=4096), True)
    timed("unwrap", sim.unwrap, True)
    timed("census", lambda: sim.census(8, 4), True)
    timed("get_state", sim.get_state, False)
    timed("host_cluster_geometry", lambda: engine.host_cluster_geometry(p, hs, a.max_size), False)
    res["baseline_wall_ms_median"] = (res["get_state"]["wall_ms_median"] +
                                      res["host_cluster_geometry"]["wall_ms_median"])
    res["geom_summary"] = out.as_dict()
    res["n_list_rows_4"] = len(sim.cluster_list(4, cap=4096))
    res["table_counts"] = {str(k): int(c) for k, c in enumerate(table["count"]) if c}
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
