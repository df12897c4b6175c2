"""Cost of the pair dynamics at C3 (1e6 proteins) after 2000 steps, next to
kmc_pair_counts, kmc_track_update and kmc_get_state measured in the same run on
the same state.  Run by hand:
  python tools/pairdyn_time.py [--workload C3] [--steps 2000] [--repeats 20] [--out profiles/pairdyn_C3.json]
For (r_max, nbins) = (300, 60) and (100, 50): the median wall time (what the
caller waits for) and HIP-event time (kmc_analysis_ms) of kmc_pd_update and of
kmc_pd_sample (both walks), of part A alone and part B alone (kmc_pd_sample
with the other part's tables NULL; each includes the binning of the current
positions), and of kmc_pair_counts AA and AB with the same r_max and nbins.
Part A counts the ordered AA + AB + BA + BB pairs, the two kmc_pair_counts
calls the unordered AA and the AB pairs: half of them and no BB.  Every repeat
steps once and updates before it samples.  In the first repeat the host twin
(kmc_host_pd_*) follows on get_state(): the arrays and the tables must be
equal, else the tool fails.
`bytes` is what a call needs at least.  Update, per protein: slot_of and the
gathered position (20 B), prev and U both ways (64 B), flags (1 B): 85 B.
Sample, per protein: U, X0, flags and the origin place in, the payload, cell
and rank out (61 B); U, cell and rank in, the current list out (40 B); each of
the three lists read once by a walk (origin list twice: 64 B): 165 B, and per
cell of the grid three 4-byte counts written or read five times (60 B).
`gbps` is that over the HIP-event time; `pairs` the pairs a call counted."""
import argparse
import ctypes as C
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


def timed(f, *args):
    t = time.perf_counter()
    out = f(*args)
    return out, (time.perf_counter() - t) * 1e3


def tables(s):
    return {k: [[int(x) for x in row] for row in getattr(s, k)] for k in ("gd", "gs") + capi.PD_COUNTS + capi.PD_SUMS}


with engine.Simulation(p) as sim:
    L = engine.load_library()
    sim.init_random()
    done = 0
    while done < a.steps:
        m = min(500, a.steps - done)
        sim.step(m)
        done += m

    for r_max, nbins in ((300.0, 60), (100.0, 50)):
        cfg = capi.pd_config(1, nbins, r_max)
        key = f"r{int(r_max)}_b{nbins}"
        sim.pd_begin(cfg)
        host = engine.HostPd(p, sim.get_state(), cfg)
        t = {k: ([], []) for k in ("pd_update", "pd_sample", "part_a", "part_b", "pair_counts_AA", "pair_counts_AB")}
        gd, gs, cu = engine._pd_tables(nbins)
        out = capi.PdOut()
        for rep in range(a.repeats):
            sim.step(1)  # returns after the stream's wait: the update starts on an idle stream
            _, wall = timed(sim.pd_update)
            t["pd_update"][0].append(wall)
            t["pd_update"][1].append(sim.analysis_ms)
            s, wall = timed(sim.pd_sample)
            t["pd_sample"][0].append(wall)
            t["pd_sample"][1].append(sim.analysis_ms)
            for name, args in (("part_a", (gd.ctypes.data, gs.ctypes.data, None)), ("part_b", (None, None, cu.ctypes.data))):
                rc, wall = timed(L.kmc_pd_sample, sim._h, C.byref(out), *args)
                assert rc == capi.KMC_OK
                t[name][0].append(wall)
                t[name][1].append(sim.analysis_ms)
            for which in ("AA", "AB"):
                pc, wall = timed(sim.pair_counts, which, r_max, nbins)
                t["pair_counts_" + which][0].append(wall)
                t["pair_counts_" + which][1].append(sim.analysis_ms)
                res.setdefault(key + "_pairs", {})[which] = int(pc.sum())
            if rep == 0:
                host.update(sim.get_state())
                U, X0, flags = sim.pd_arrays()
                if not (np.array_equal(U, host.arrays.U) and np.array_equal(X0, host.arrays.X0) and
                        np.array_equal(flags, host.arrays.flags)):
                    sys.exit(f"{key}: the device's arrays differ from the host twin's")
                if tables(s) != tables(host.sample()):
                    sys.exit(f"{key}: the device's tables differ from the host twin's")
        r = {"equal_to_host_twin": True, "ncx": s.ncx, "ncy": s.ncy,
             "pairs_a": int(s.gd.sum() + s.gs.sum()), "pairs_b": int(s.n_pairs.sum()), "valid_b": int(s.n_valid.sum())}
        nbytes = {"pd_update": 85 * n, "pd_sample": 165 * n + 60 * s.ncx * s.ncy}
        for name, (wall, dev) in t.items():
            r[name] = {"wall_ms": med(wall), "device_ms": med(dev)}
            if name in nbytes:
                r[name]["bytes"] = nbytes[name]
                r[name]["gbps"] = nbytes[name] / (statistics.median(dev) * 1e-3) / 1e9
        r["part_a_over_pair_counts"] = r["part_a"]["device_ms"]["median"] / (
            r["pair_counts_AA"]["device_ms"]["median"] + r["pair_counts_AB"]["device_ms"]["median"])
        res[key] = r
        sim.pd_end()

    # the yardsticks, in the same run
    sim.track_begin()
    sim.track_update()
    wall, dev = [], []
    for _ in range(a.repeats):
        sim.step(1)
        _, w = timed(sim.track_update)
        wall.append(w)
        dev.append(sim.analysis_ms)
    res["track_update"] = {"wall_ms": med(wall), "device_ms": med(dev)}
    sim.get_state()
    wall = [timed(sim.get_state)[1] for _ in range(a.repeats)]
    res["get_state"] = {"wall_ms": med(wall)}
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
