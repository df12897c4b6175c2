"""Cost of the lag correlator at C3 (1e6 proteins) after 2000 steps, next to
kmc_track_update and kmc_get_state measured in the same run.  Run by hand:
  python tools/lag_time.py [--workload C3] [--steps 2000] [--repeats 20] [--out profiles/lag_C3.json]
For (levels, slots) = (1, 8) and (12, 8), with nq = 0 and 2 multipliers: the
median wall time (what the caller waits for) and HIP-event time
(kmc_analysis_ms) of kmc_lag_update at
  common    an update at which only level 0 fires, with all its 8 tasks (odd n > 8),
  all_fire  the update at which every level reachable in the window fires: the
            window is 64 updates, so n = 64 (levels 0..6 store an origin, levels
            0..3 hold stored origins to correlate with: 20 tasks), (12, 8) only,
and of kmc_lag_sample.  Every repeat begins a new recorder and walks the
window, one step an update.  In the first repeat the host twin
(kmc_host_lag_*) walks along on get_state(): the arrays after every update and
the table at the window's end must be equal, else the tool fails.
`bytes` is what an update needs at least: per protein (2 + tasks) * 16 B (U in
and out, one origin a task; the origins stored on top: 16 B a firing level)
+ 40 B (prev both ways, slot_of, last_event) and the gathered position and
links; `gbps` is that over the HIP-event time."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = "kmc-with-a-diffusion-reaction-algorithm_amd"
capi = importlib.import_module(PKG + ".capi")
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
res = {"workload": a.workload, "n_a": p.n_a, "n_b": p.n_b, "steps": a.steps, "repeats": a.repeats, "every": 1}


def med(x):
    return {"median": statistics.median(x), "min": min(x), "count": len(x)}


def same(s, t):
    return all(np.array_equal(getattr(s, k), getattr(t, k)) for k in
               capi.LAG_COUNTS + capi.LAG_SUMS + ("fs", "n_pairs"))


with engine.Simulation(p) as sim:
    sim.init_random()
    done = 0
    while done < a.steps:
        m = min(500, a.steps - done)
        sim.step(m)
        done += m

    for levels, slots, window in ((1, 8, 16), (12, 8, 64)):
        for h in ((), (1, 3)):
            cfg = capi.lag_config(1, levels, slots, h=h)
            key = f"L{levels}_P{slots}_nq{len(h)}"
            kinds = {"common": ([], [], 8, 1), "all_fire": ([], [], None, None)}
            for rep in range(a.repeats):
                sim.lag_begin(cfg)
                host = engine.HostLag(p, sim.get_state(), cfg) if rep == 0 else None
                for k in range(1, window + 1):
                    sim.step(1)  # returns after the stream's wait: the update starts on an idle stream
                    t = time.perf_counter()
                    info = sim.lag_update()
                    wall = (time.perf_counter() - t) * 1e3
                    dev = sim.analysis_ms
                    fired = next(l for l in range(levels + 1) if l == levels or k % (1 << l))  # levels 0..fired-1
                    if k % 2 == 1 and k > slots:
                        kinds["common"][0].append(wall)
                        kinds["common"][1].append(dev)
                        assert info.n_tasks == slots
                    if levels > 1 and k == window:
                        kinds["all_fire"][0].append(wall)
                        kinds["all_fire"][1].append(dev)
                        kinds["all_fire"] = kinds["all_fire"][:2] + (int(info.n_tasks), fired)
                    if host is not None:
                        want = host.update(sim.get_state())
                        U, le = sim.lag_arrays()
                        if not (np.array_equal(U, host.arrays.U) and np.array_equal(le, host.arrays.last_event) and
                                (info.n_tasks, info.n_events) == (want.n_tasks, want.n_events)):
                            sys.exit(f"{key}: the device's arrays differ from the host twin's at update {k}")
                if host is not None and not same(sim.lag_sample(), host.sample()):
                    sys.exit(f"{key}: the device's table differs from the host twin's")
            r = {"equal_to_host_twin": True, "window": window}
            for name, (wall, dev, tasks, fired) in kinds.items():
                if not wall:
                    continue
                nbytes = ((2 + tasks) * 16 + 16 * fired + 40 + 16 + 12) * n
                r[name] = {"tasks": tasks, "levels_fired": fired, "wall_ms": med(wall), "device_ms": med(dev),
                           "bytes": nbytes, "gbps": nbytes / (statistics.median(dev) * 1e-3) / 1e9}
            wall, dev = [], []
            for _ in range(a.repeats):
                t = time.perf_counter()
                s = sim.lag_sample()
                wall.append((time.perf_counter() - t) * 1e3)
                dev.append(sim.analysis_ms)
            r["lag_sample"] = {"wall_ms": med(wall), "device_ms": med(dev), "rows": s.rows}
            r["n_clean"], r["n_all"], r["n_far"] = int(s.n_clean.sum()), int(s.n_all.sum()), int(s.n_far.sum())
            res[key] = r
            sim.lag_end()

    # the yardsticks, in the same run
    sim.track_begin()
    sim.track_update()
    wall, dev = [], []
    for _ in range(a.repeats):
        sim.step(1)
        t = time.perf_counter()
        sim.track_update()
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(sim.analysis_ms)
    res["track_update"] = {"wall_ms": med(wall), "device_ms": med(dev)}
    sim.get_state()
    wall = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        sim.get_state()
        wall.append((time.perf_counter() - t) * 1e3)
    res["get_state"] = {"wall_ms": med(wall)}
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
