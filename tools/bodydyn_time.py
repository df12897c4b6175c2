"""Cost of the body dynamics at C3 (1e6 proteins) after 2000 steps, next to
kmc_pd_update, kmc_cluster_geometry and kmc_get_state measured in the same run
on the same state, and on the brick-wall gel (one body of 8192 members).  Run
by hand:
  python tools/bodydyn_time.py [--workload C3] [--steps 2000] [--repeats 20] [--out profiles/bodydyn_C3.json]
The median wall time (what the caller waits for) and HIP-event time
(kmc_analysis_ms) of kmc_bd_begin, kmc_bd_update, kmc_bd_sample — with its
components, reduction and finish apart (kmc_bd_sample_ms) — and kmc_bd_bodies,
of kmc_pd_update (the same per-protein step without the links), of
kmc_cluster_geometry (per-cluster sums by per-member atomics: five launches and
the table) and kmc_components.  Every repeat steps once and updates before it
samples.  In the first repeat the host twin (kmc_host_bd_*) follows on
get_state(): the arrays, the table and the list must be equal, else the tool
fails.
`bytes` is what a call needs at least.  Update, per protein: slot_of and the
gathered position and links (32 B), prev and U both ways (64 B), the stored
links (12 B), flags (1 B): 109 B.  Reduce, per protein: the list entry (4 B),
the gathered label, U, X0, D0, flags and current label (57 B): 61 B, and per
body the two starts and seven words out (64 B).  `gbps` is that over the
HIP-event time."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "kmc-with-a-diffusion-reaction-algorithm_amd"
capi = importlib.import_module(PKG + ".capi")
engine = importlib.import_module(PKG + ".engine")
workloads = importlib.import_module(PKG + ".workloads")

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="C3")
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--max-size", type=int, default=64)
ap.add_argument("--gel", action="store_true", help="also the brick-wall gel of tests/_geometry.py (needs tests/)")
ap.add_argument("--out", default=None)
a = ap.parse_args()


def med(x):
    return {"median": statistics.median(x), "min": min(x), "count": len(x)}


def timed(f, *args):
    t = time.perf_counter()
    out = f(*args)
    return out, (time.perf_counter() - t) * 1e3


def table(s):
    return {k: [[int(x) for x in row] for row in getattr(s, k)] for k in capi.BD_COUNTS + capi.BD_SUMS}


def measure(sim, p, cfg, repeats, stepping, others):
    n = p.n_a + p.n_b
    _, wall = timed(sim.bd_begin, cfg)
    r = {"bd_begin": {"wall_ms": wall, "device_ms": sim.analysis_ms}}
    host = engine.HostBd(p, sim.get_state(), cfg)
    names = ["bd_update", "bd_sample", "bd_components", "bd_reduce", "bd_finish", "bd_bodies"] + list(others)
    t = {k: ([], []) for k in names}
    s = None
    for rep in range(repeats):
        if stepping:
            sim.step(cfg.every)  # returns after the stream's wait: the update starts on an idle stream
            _, wall = timed(sim.bd_update)
            t["bd_update"][0].append(wall)
            t["bd_update"][1].append(sim.analysis_ms)
        s, wall = timed(sim.bd_sample)  # (two calls: the first fetches the configuration only)
        t["bd_sample"][0].append(wall)
        t["bd_sample"][1].append(sim.analysis_ms)
        for name, ms in zip(("bd_components", "bd_reduce", "bd_finish"), sim.bd_sample_ms()):
            t[name][1].append(ms)
        rows, wall = timed(sim.bd_bodies, 2)
        t["bd_bodies"][0].append(wall)
        t["bd_bodies"][1].append(sim.analysis_ms)
        for name, f in others.items():
            _, wall = timed(f)
            t[name][0].append(wall)
            t[name][1].append(sim.analysis_ms)
        if rep == 0:
            hs = sim.get_state()
            if stepping:
                host.update(hs)
            U, X0, flags, label, D0 = sim.bd_arrays()
            h = host.arrays
            if not (np.array_equal(U, h.U) and np.array_equal(flags, h.flags) and np.array_equal(label, h.label) and
                    np.array_equal(D0, h.D0)):
                sys.exit("the device's arrays differ from the host twin's")
            if table(s) != table(host.sample(hs)) or not np.array_equal(rows, host.bodies(hs, 2)):
                sys.exit("the device's table or list differs from the host twin's")
    n_bodies = s.total_bodies
    nbytes = {"bd_update": 109 * n, "bd_reduce": 61 * n + 64 * n_bodies}
    r.update(equal_to_host_twin=True, n=n, n_bodies=n_bodies, largest=int(max(rows["n_r"] + rows["n_l"], default=1)),
             n_valid=int(sum(int(x) for row in s.n_valid for x in row)),
             n_rot=int(sum(int(x) for row in s.n_rot for x in row)))
    for name, (wall, dev) in t.items():
        if not dev:
            continue
        r[name] = {"device_ms": med(dev)}
        if wall:
            r[name]["wall_ms"] = med(wall)
        if name in nbytes:
            r[name]["bytes"] = nbytes[name]
            r[name]["gbps"] = nbytes[name] / (statistics.median(dev) * 1e-3) / 1e9
    r["reduce_ns_per_entry"] = statistics.median(t["bd_reduce"][1]) * 1e6 / n
    sim.bd_end()
    return r


p = workloads.params(a.workload)
res = {"workload": a.workload, "n_a": p.n_a, "n_b": p.n_b, "steps": a.steps, "repeats": a.repeats, "every": 1,
       "max_size": a.max_size}
with engine.Simulation(p) as sim:
    sim.init_random()
    done = 0
    while done < a.steps:
        m = min(500, a.steps - done)
        sim.step(m)
        done += m
    sim.pd_begin(capi.pd_config(1, 10, 100.0))

    def pd_update():  # on the stride: the recorders share the step of the repeat
        sim.pd_update()

    others = {"pd_update": pd_update, "cluster_geometry": lambda: sim.cluster_geometry(a.max_size),
              "components": sim.components}
    res["run"] = measure(sim, p, capi.bd_config(1, a.max_size), a.repeats, True, others)
    sim.pd_end()
    sim.get_state()
    wall = [timed(sim.get_state)[1] for _ in range(a.repeats)]
    res["get_state"] = {"wall_ms": med(wall)}

if a.gel:
    sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")]
    from _geometry import lattice_state
    pg, hs = lattice_state(False, False)
    with engine.Simulation(pg) as sim:
        sim.set_state(hs)
        others = {"cluster_geometry": lambda: sim.cluster_geometry(a.max_size), "components": sim.components}
        res["gel"] = measure(sim, pg, capi.bd_config(1, a.max_size), a.repeats, False, others)
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
