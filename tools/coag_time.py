"""Cost of the cluster growth recorder at C3 (1e6 proteins) after 2000 steps, with
kmc_oligomer_census and kmc_kin_update measured in the same run as yardsticks:
an update contains one an_components (the census' own labelling) and a second
union-find over the kept bonds, the kinetics update is one pass over the
receptors.  Run by hand:
  python tools/coag_time.py [--workload C3] [--steps 2000] [--repeats 20] [--max-size 16] [--out profiles/coag_C3.json]
For cf_update, census and kin_update: the median and minimum wall time of a
call over the repeats (what the caller waits for: launches, the wait, the
result copies) and the HIP-event time of the call's kernels (kmc_analysis_ms);
for cf_sample, which launches nothing (two calls and the table copies), the
wall time alone.  One step is taken before every update, as a run that
records events exact up to simultaneous ones does."""
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
ap.add_argument("--max-size", type=int, default=16)
ap.add_argument("--out", default=None)
a = ap.parse_args()

p = workloads.params(a.workload)
res = {"workload": a.workload, "n_a": p.n_a, "n_b": p.n_b, "steps": a.steps, "repeats": a.repeats,
       "max_size": a.max_size}
with engine.Simulation(p) as sim:
    sim.init_random()
    done = 0
    while done < a.steps:
        m = min(500, a.steps - done)
        sim.step(m)
        done += m
    sim.cf_begin(a.max_size)
    sim.kin_begin()

    def timed(name, f, before=None, device=True):
        f()  # warm
        wall, dev = [], []
        for _ in range(a.repeats):
            if before:
                before()
            t = time.perf_counter()
            f()
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(sim.analysis_ms)
        res[name] = {"wall_ms_median": statistics.median(wall), "wall_ms_min": min(wall)}
        if device:
            res[name].update(device_ms_median=statistics.median(dev), device_ms_min=min(dev))

    # step() returns after kmc_step has waited for the stream (its records are copied out), so each
    # call's wall time starts on an idle stream; the calls are timed in turns over the same steps
    step = lambda: sim.step(1)  # noqa: E731
    timed("cf_update", sim.cf_update, before=step)
    timed("census", lambda: sim.census(8, 8), before=step)
    timed("kin_update", sim.kin_update, before=step)
    timed("cf_update_again", sim.cf_update, before=step)
    timed("cf_sample", sim.cf_sample, device=False)
    out, t = sim.cf_sample()
    res["out"] = out.as_dict()
    res["merge_pieces"] = t.merge_pieces.tolist()
    res["frag_pieces"] = t.frag_pieces.tolist()
    res["n_s"] = t.n_s.tolist()
    res["ratio_to_census_device_median"] = res["cf_update"]["device_ms_median"] / res["census"]["device_ms_median"]
    res["ratio_to_kin_update_device_median"] = (res["cf_update"]["device_ms_median"]
                                                / res["kin_update"]["device_ms_median"])
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
