"""Cost of the displacement tracking at C3 (1e6 proteins) after 2000 steps, against
get_state() — the only route to displacements before it.  Run by hand:
  python tools/dynamics_time.py [--workload C3] [--steps 2000] [--repeats 20] [--out profiles/dynamics_C3.json]
For track_update and track_sample (r_max 200, 64 bins): the median and minimum
wall time of a call over the repeats (what the caller waits for: launches, the
wait, the result copies) and the HIP-event time of the call's kernels
(kmc_analysis_ms); 20 steps are taken between the updates, as a tracked run
does, so every update sees moved proteins.  get_state() is a device re-order,
four copies and a host pass: wall time is its only measure.  `update_bytes` is
the traffic the update's kernel needs at least per call (the tracker's arrays
once each way, the gathered position and links)."""
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
n = p.n_a + p.n_b
res = {"workload": a.workload, "n_a": p.n_a, "n_b": p.n_b, "steps": a.steps, "repeats": a.repeats}
with engine.Simulation(p) as sim:
    sim.init_random()
    done = 0
    while done < a.steps:
        m = min(500, a.steps - done)
        sim.step(m)
        done += m
    sim.track_begin()

    def timed(name, f, device, before=None):
        f()  # warm
        wall, dev = [], []
        for _ in range(a.repeats):
            if before:
                before()
            t = time.perf_counter()
            f()
            wall.append((time.perf_counter() - t) * 1e3)
            if device:
                dev.append(sim.analysis_ms)
        res[name] = {"wall_ms_median": statistics.median(wall), "wall_ms_min": min(wall)}
        if device:
            res[name].update(device_ms_median=statistics.median(dev), device_ms_min=min(dev))

    # step() returns after kmc_step has waited for the stream (its records are copied out), so the
    # update's wall time starts on an idle stream
    timed("track_update", sim.track_update, True, before=lambda: sim.step(20))
    timed("track_sample_64", lambda: sim.track_sample(200.0, 64), True)
    timed("get_state", sim.get_state, False)
    info = sim.track_update()
    out, vh = sim.track_sample(200.0, 64)
    res["info"] = info.as_dict()
    res["sample"] = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in out.as_dict().items()}
    res["vanhove_counted"] = int(vh.sum())
    # per protein: prev 16 + 16, u 16 + 16, flags 1 + 1, origin links 12, slot_of 4, position 16, links 12
    res["update_bytes"] = 110 * n
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
