"""The re-sort's hand-written radix sort and scan (kmc_kernels.hip
k_rs_hist / k_rs_scatter / k_scan_*, kmc_engine.hip radix_sort / dev_scan).

With KMC_DEBUG_SYNC=1 the engine checks every re-sort on the host: the
sorted slot keys non-decreasing, equal keys in input order (a stable sort),
each kind's values a permutation, and the home list's cell starts the
exclusive scan of its counts — a failure is an engine error.  Nothing of the
trajectory depends on the slot order, so a run re-sorted every
7 steps under each grouping mode must equal the default run in every bond.dat
record and full-state hash; sizes are ragged against the sort's 4096-key
tiles and the keys span several 8-bit passes.  A second test takes the sizes at
the tiles' edges: one partial tile, exactly one full tile, and 257 tiles, where
k_rs_rows needs a second iteration of 256 tiles with a carry."""
import math

import numpy as np
import pytest

from _kmc import DENSE, engine

pytestmark = pytest.mark.gpu


RS_TILE = 4096  # kmc_kernels.hip: keys per workgroup of the radix sort; k_rs_rows takes 256 tiles an iteration


def _params(n_a, n_b, seed, **kw):
    L = 5773.0 * math.sqrt((n_a + n_b) / 2000)
    return engine.capi.default_params(n_a=n_a, n_b=n_b, box_x=L, box_y=L, box_z=1000.0, seed=seed, **kw)


def _run(monkeypatch, p, st, steps, env, every=10):
    for k in ("KMC_RESORT", "KMC_GROUP_SORT", "KMC_DEBUG_SYNC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    obs, hashes = [], []
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        for _ in range(steps // every):
            obs.append(sim.step(every))
            hashes.append(engine.state_hash(p, sim.get_state()))
    return np.concatenate(obs), hashes


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_a,n_b", [(9000, 3001), (30001, 10003)])
def test_resort_sort_checked_and_trajectory_unchanged(monkeypatch, n_a, n_b):
    p = _params(n_a, n_b, seed=5)
    st = engine.host_init_random(p)
    # an evolved state: complexes and dimers give the grouped keys equal runs
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        sim.step(2000)
        st = sim.get_state()
    assert int(st.counters[0]) > 0
    want, hw = _run(monkeypatch, p, st, 60, {})
    for group in ("0", "1", "2"):
        got, hg = _run(monkeypatch, p, st, 60, {"KMC_RESORT": "7", "KMC_GROUP_SORT": group, "KMC_DEBUG_SYNC": "1"})
        assert np.array_equal(got, want), group
        assert hg == hw, group


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_a,n_b,groups", [(150, 50, "012"), (3000, 1096, "012"), (786_500, 262_200, "02")])
def test_resort_at_the_tile_edges(monkeypatch, n_a, n_b, groups):
    # one partial tile; exactly one full tile; 257 tiles.  A short evolution at the dense rates instead of 2000
    # default-rate steps, and one window of 30 steps re-sorted every 10 (before steps 2, 12 and 22) with one state
    # read at its end: the host check is O(N) a re-sort
    n = n_a + n_b
    tiles = (n + RS_TILE - 1) // RS_TILE
    assert (tiles == 1 and n < RS_TILE) or n == RS_TILE or tiles > 256
    p = _params(n_a, n_b, seed=5, **{k: v for k, v in DENSE.items() if not k.startswith("box_")})
    st = engine.host_init_random(p)
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        sim.step(1000)
        st = sim.get_state()
    assert int(st.counters[0]) > 0
    want, hw = _run(monkeypatch, p, st, 30, {}, every=30)
    for group in groups:
        got, hg = _run(monkeypatch, p, st, 30, {"KMC_RESORT": "10", "KMC_GROUP_SORT": group, "KMC_DEBUG_SYNC": "1"},
                       every=30)
        assert np.array_equal(got, want), group
        assert hg == hw, group
