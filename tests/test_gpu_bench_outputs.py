"""A plain `bench.py` run (no --full) and its --dump-outputs files: the line
carries the headline figures and none of the --full measurements, the timed
window is the same stretch of the trajectory a --full run times (placement,
then 2 W + K + E steps before it ends), and the dumped arrays are what that
window returned: its per-step records and the state it left, equal to the
keyed oracle's bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _kmc import O, REPO, capi, engine, workloads

BENCH = os.path.join(REPO, "bench.py")
WARMUP, STEPS, EVOLVE = 5, 20, 300


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def test_profile_needs_full():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--profile"], capture_output=True, text=True,
                       env=_env(), timeout=60)
    assert r.returncode != 0
    assert "--full" in r.stderr


@pytest.mark.gpu
@pytest.mark.timeout(200)
def test_plain_run_line_and_dumped_outputs_equal_oracle(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--workload", "C1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--evolve", str(EVOLVE), "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=_env(), timeout=180)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    p = workloads.params("C1", seed=1, replica=0)
    n = p.n_a + p.n_b
    assert d["full"] is False and d["steps"] == STEPS and d["warmup"] == WARMUP
    assert d["unit"] == "particle-updates/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["value"] == pytest.approx(n * STEPS / (d["ms_per_step"] * STEPS / 1e3), rel=1e-9)
    # nothing of a --full run
    assert d["cpu_baseline"] is None and d["config"]["ms_per_step_fresh"] is None
    assert "kernel" not in d["roofline"] and "by_kernel" not in d["roofline"]
    total = 2 * WARMUP + 2 * STEPS + EVOLVE
    assert d["config"]["timed_from_step"] + STEPS == total

    o = O.Oracle(p, rng_mode=O.RNG_KEYED, nbmode=O.NB_CELLS)
    o.set_state(engine.host_init_random(p))
    obs, _ = o.step(total, want_hashes=False)
    st = o.get_state()

    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 2**20
    fields = [f for f in capi.OBS_DTYPE.names if f != "reserved"]
    want = np.stack([obs[f].astype(np.float64) for f in fields], axis=1)[-STEPS:]
    assert np.array_equal(got["obs"], want)
    # one rank: the ensemble reduction is this rank's own series
    assert np.array_equal(got["ensemble_sums"][:, 3], want[:, fields.index("bond_num")])
    assert np.array_equal(got["state_counters"], np.append(st.counters.astype(np.float64), float(total)))
    for kind, pos, ints in (("receptors", st.ra, st.a_int), ("ligands", st.rb, st.b_int)):
        ids = got[f"state_{kind}_ids"].astype(np.int64)
        assert len(ids) == pos.shape[1] and np.array_equal(ids, np.arange(len(ids)))
        assert np.array_equal(got[f"state_{kind}_beads"], pos[:, ids].T)
        assert np.array_equal(got[f"state_{kind}_ints"], ints[:, ids].T.astype(np.float64))
