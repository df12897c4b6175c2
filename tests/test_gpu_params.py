"""GPU parity away from the reference's default parameters.

kmc_create accepts any radius and cutoff up to the reference's, any time step
and any mobility; the kernels' reaches, pair-filter constants, refinement
margins and the outlier list were derived for the defaults ("smaller values
only shrink every reach").  Here the engine runs the golden scenarios `small`
(shrunken radii and cutoffs, other angle windows, a rectangular box), `fast`
(a long step, other mobilities) and `pai` (another truncation of pi, wider
angle windows), which tests/test_oracle_golden.py pins to the reference, and
`stride` (a 400 ns step: outliers without a debug knob) against the keyed CPU
oracle.  Every comparison is an equality: each bond.dat record and the FNV
hash of the full state.  Also: one-species and one-protein populations, and
what kmc_create accepts and refuses.
"""
import re

import numpy as np
import pytest

from _kmc import (COVERAGE, O, STRIDE, capi, compare_stepwise, engine, golden_state, params, scenario_params,
                  scenarios, stats_delta)

pytestmark = pytest.mark.gpu

NAMES = [n for n in ("small", "fast", "pai") if n in scenarios()]
LATE = {"small": 3000, "fast": 3000, "pai": 3000}  # the golden dump each late window starts from
WINDOW = 1200


@pytest.fixture(scope="module")
def late_runs():
    """Per scenario: (params, state the reference dumped, the keyed oracle's records and hashes over the
    window from it, the oracle's event counts over the window) — computed once, shared by the knob variants."""
    cache = {}

    def get(name):
        if name not in cache:
            p = scenario_params(name, seed=17)
            st, _ = golden_state(name, LATE[name])
            o = O.Oracle(p, rng_mode=O.RNG_KEYED)
            o.set_state(st)
            before = o.stats()
            obs, hashes = o.step(WINDOW)
            cache[name] = (p, st, obs, hashes, stats_delta(before, o.stats()))
        return cache[name]

    return get


# ---------------------------------------------------------------- 1. stepwise parity, 150 + 50
@pytest.mark.parametrize("name", NAMES)
def test_stepwise_from_placement(name):
    p = scenario_params(name, seed=23)
    o = compare_stepwise(p, 1500)
    ev = o.stats()
    assert ev["reject"] > 0 and ev["mono"] > 0 and ev["free_b"] > 0, ev


@pytest.mark.parametrize("name", NAMES)
def test_stepwise_from_late_dump(name, late_runs):
    p, st, obs, hashes, ev = late_runs(name)
    assert int(st.counters[0]) > 0, "the dump holds no bond"
    for k in COVERAGE:
        assert ev[k] > 0, (k, ev)
    compare_stepwise(p, WINDOW, init_state=st, oracle_run=(obs, hashes))


# ---------------------------------------------------------------- 2. the non-default code paths, off-default geometry
KNOBS = [("KMC_COL_REFINE", "0"), ("KMC_RXN_REFINE", "0"), ("KMC_DEBUG_TCAP", "0"), ("KMC_DEBUG_HTAG", "0"),
         ("KMC_TILE", "2"), ("KMC_RESORT", "7"), ("KMC_GRAPH", "0"), ("KMC_DEBUG_RECS", "1")]


@pytest.mark.parametrize("knob,value", KNOBS, ids=[f"{k}={v}" for k, v in KNOBS])
def test_knob_small_geometry(monkeypatch, late_runs, knob, value):
    p, st, obs_o, hashes, ev = late_runs("small")
    assert ev["rl"] > 0 and ev["laydown"] > 0 and ev["complex"] > 0 and ev["reject"] > 0, ev
    monkeypatch.setenv(knob, value)
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        obs = np.concatenate([sim.step(n) for n in (1, 2, 597, WINDOW - 600)])
        h = engine.state_hash(p, sim.get_state())
    assert np.array_equal(obs, obs_o)
    assert h == int(hashes[-1])


def test_rxn_refinement_engages_small_geometry(monkeypatch, capfd, late_runs):
    # sites_ok must accept binding sites built with the smaller ra_radius, or the R–L refinement is off
    # for every state at these radii and the knob test above compares the unrefined path with itself
    p, st, obs_o, hashes, _ = late_runs("small")
    monkeypatch.setenv("KMC_DEBUG_CAND", "1")
    monkeypatch.setenv("KMC_DEBUG_COUNTS", "1")
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        obs = np.concatenate([sim.step(100) for _ in range(6)])
        h = engine.state_hash(p, sim.get_state())
    assert np.array_equal(obs, obs_o[:600]) and h == int(hashes[599])
    lines = [x.split() for x in capfd.readouterr().err.splitlines() if "refined-out" in x]
    out = [int(f[f.index("refined-out") + 1]) for f in lines]
    final = [int(f[f.index("final") + 1]) for f in lines]
    print("refined-out", out, "final", final)
    assert len(out) == 6 and max(out) > 0 and max(final) > 0


# ---------------------------------------------------------------- 3. mid size, the cell oracle
MID = dict(n_a=4000, n_b=1500, box_x=7500.0, box_y=4800.0)  # the area of test_larger_box_cell_oracle's 6000 Å box


def _mid_params(name):
    if name == "stride":
        return params(seed=9, box_z=250.0, **MID, **STRIDE)
    return scenario_params(name, seed=9, **MID)


def _chunks_vs_oracle(p, st, steps):
    o = O.Oracle(p, nbmode=O.NB_CELLS)
    o.set_state(st)
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        obs = sim.step(steps)
        h = engine.state_hash(p, sim.get_state())
    obs_o, _ = o.step(steps, want_hashes=False)
    assert np.array_equal(obs, obs_o)
    assert h == o.hash()
    return o


@pytest.mark.parametrize("name", ["small", "fast"])
def test_mid_size_from_placement(name):
    p = _mid_params(name)
    _chunks_vs_oracle(p, engine.host_init_random(p), 300)


@pytest.mark.parametrize("name", ["small", "fast"])
def test_mid_size_from_evolved_state(name):
    # tiles, home list, buckets and complexes see the changed geometry together
    p = _mid_params(name)
    with engine.Simulation(p) as sim:
        sim.set_state(engine.host_init_random(p))
        last = sim.step(3000)[-1]
        st = sim.get_state()
    assert engine.host_validate(p, st) == capi.KMC_OK
    assert int(st.counters[0]) > 0 and int(st.counters[1]) > 0, st.counters  # bonds, R–L bonds
    assert last["tot_cluster_num"] > 0 and last["protein_num_in_max_complex"] >= 2, last
    o = _chunks_vs_oracle(p, st, 150)
    ev = o.stats()
    assert ev["complex"] > 0 and ev["reject"] > 0, ev


def test_stride_outliers_without_debug_knob(monkeypatch, capfd):
    # amp_b = 44 Å, amp_a = 16 Å a step: proteins leave the neighbourhood of their home cell between
    # the default re-sorts, so the outlier list and the tiles' buckets fill in an ordinary run
    monkeypatch.setenv("KMC_DEBUG_COUNTS", "1")
    p = params(n_a=20000, n_b=7000, seed=9, box_x=14000.0, box_y=14000.0, box_z=250.0, **STRIDE)
    for r in ("ass_rate", "mono_cis_ass_rate", "cis_ass_rate", "diss_rate", "mono_cis_diss_rate", "cis_diss_rate"):
        assert getattr(p, r) * p.time_step < 1.0
    st = engine.host_init_random(p)
    o = O.Oracle(p, nbmode=O.NB_CELLS)
    o.set_state(st)
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        obs = np.concatenate([sim.step(25) for _ in range(6)])
        h = engine.state_hash(p, sim.get_state())
    obs_o, _ = o.step(150, want_hashes=False)
    assert np.array_equal(obs, obs_o)
    assert h == o.hash()
    err = capfd.readouterr().err
    outl = [int(x) for x in re.findall(r"outliers (\d+)", err)]
    print("outliers", outl, "replays", re.findall(r"replays (\d+)", err)[-1:])
    assert outl and max(outl) > 10, f"no outliers at a 44 Å stride: {outl}"
    assert obs_o[-1]["bond_num"] > 0


# ---------------------------------------------------------------- 4. degenerate populations
TINY_BOX = dict(box_x=400.0, box_y=300.0, box_z=250.0)
TINY = [(40, 0), (0, 30), (1, 0), (0, 1), (1, 1), (2, 1)]


def _ligand_lattice(p):
    """n_b = 30 ligands lying flat (the template's own orientation, main.cpp:1157-1179) on a 3 x 2 x 5
    lattice: 133 Å and 150 Å apart in x and y — beyond the 2 rb (1 + 2 / sqrt 3) = 129 Å that separates any
    two ligands' subunits —, the layers 61 Å apart, one subunit diameter."""
    rb, s3 = p.rb_radius, np.sqrt(3.0)
    tpl = {(1, 1): (0, 0, 0), (1, 2): (0, 0, rb), (2, 1): (0, rb * 2 / s3, 0), (2, 2): (0, rb * (2 / s3 + 1), 0),
           (3, 1): (-rb, -rb / s3, 0), (3, 2): (-rb * (s3 / 2 + 1), -rb / s3 - rb / 2, 0),
           (4, 1): (rb, -rb / s3, 0), (4, 2): (rb * (s3 / 2 + 1), -rb / s3 - rb / 2, 0)}
    st = capi.HostState(0, p.n_b)
    b = 0
    for l in range(5):
        for j in range(2):
            for i in range(3):
                c = (-p.box_x / 2 + (i + 0.5) * p.box_x / 3, -p.box_y / 2 + (j + 0.5) * p.box_y / 2, 3.0 + 61.0 * l)
                for (jj, kk), off in tpl.items():
                    for ax in range(3):
                        st.rb[((jj - 1) * 2 + (kk - 1)) * 3 + ax, b] = c[ax] + off[ax]
                b += 1
    assert b == p.n_b
    return st


def _tiny_state(p):
    """The library's placement; for 30 ligands alone a lattice.  Random sequential placement cannot put
    30 ligands into this box, with or without receptors: each excludes a sphere of 129 Å around its centre
    (main.cpp:372), 30 such spheres are more than a random sequential packing holds in 400 x 300 x 250 Å,
    and the sampler — the oracle's and the library's alike — ends with KMC_ERR_PLACEMENT."""
    if (p.n_a, p.n_b) == (0, 30):
        return _ligand_lattice(p)
    return engine.host_init_random(p)


@pytest.mark.parametrize("n_a,n_b", TINY)
def test_degenerate_populations_stepwise(n_a, n_b):
    p = params(n_a=n_a, n_b=n_b, seed=5, **TINY_BOX)
    st = _tiny_state(p)
    assert engine.host_validate(p, st) == capi.KMC_OK
    o = compare_stepwise(p, 200, init_state=st)
    assert o.current_step == 200


@pytest.mark.parametrize("n_a,n_b", [(40, 0), (0, 30)])
def test_one_species_analysis_and_resume(tmp_path, n_a, n_b):
    p = params(n_a=n_a, n_b=n_b, seed=5, **TINY_BOX)
    st = _tiny_state(p)
    o = O.Oracle(p)
    o.set_state(st)
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        sim.step(50)
        row, mem = sim.clusters()
        row_o, mem_o = (o.step(50, want_hashes=False), o.clusters())[1]
        assert np.array_equal(row, row_o) and np.array_equal(mem, mem_o)
        assert len(row) == n_b and int(row.sum()) == n_b  # every ligand its own cluster, no receptor in any
        hist, cen = sim.census(3, 3)
        # every protein is a component of one: n_a monomers of a receptor, n_b of a ligand
        assert hist[1, 0] == n_a and hist[0, 1] == n_b and int(hist.sum()) == n_a + n_b
        path = str(tmp_path / "state.kmc")
        sim.save_state(path)
        obs_a = sim.step(50)
        h_a = engine.state_hash(p, sim.get_state())
    with engine.Simulation(p) as sim2:
        sim2.load_state(path)
        assert sim2.current_step == 50
        obs_b = sim2.step(50)
        assert np.array_equal(obs_a, obs_b)
        assert engine.state_hash(p, sim2.get_state()) == h_a
    obs_o, _ = o.step(50, want_hashes=False)
    assert np.array_equal(obs_a, obs_o) and o.hash() == h_a


# ---------------------------------------------------------------- 5. what kmc_create accepts
BOUNDED = {"ra_radius": 20.0, "rb_radius": 30.0, "bond_dist_cutoff": 18.0, "cis_dist_cutoff": 15.0}
DOUBLES = [n for n, t in capi.Params._fields_ if t is capi.C.c_double]
POSITIVE = ["box_x", "box_y", "box_z", "time_step", "pai", "ra_radius", "rb_radius", "bond_dist_cutoff",
            "cis_dist_cutoff", "bond_thetapd_cutoff", "bond_thetaot_cutoff", "cis_thetaot_cutoff"]
NON_NEGATIVE = [n for n in DOUBLES if n not in POSITIVE]


def _create_rc(**kw):
    p = params(n_a=3, n_b=2, **{**TINY_BOX, **kw})
    host = engine.host_check_params(p)
    try:
        engine.Simulation(p).close()
        rc = capi.KMC_OK
    except engine.KmcError as e:
        rc = e.code
    assert rc == host, f"kmc_create {rc} and kmc_host_check_params {host} disagree for {kw}"
    return rc


def test_create_field_lists_cover_every_double():
    assert len(DOUBLES) == 26 and sorted(POSITIVE + NON_NEGATIVE) == sorted(DOUBLES)
    assert len(NON_NEGATIVE) == 14  # 8 D / rot_D and 6 rates


@pytest.mark.parametrize("field", list(BOUNDED))
def test_create_bound_is_inclusive(field):
    b = BOUNDED[field]
    assert _create_rc(**{field: b}) == capi.KMC_OK
    assert _create_rc(**{field: float(np.nextafter(b, np.inf))}) == capi.ERR_ARG
    assert _create_rc(**{field: float(np.nextafter(b, 0.0))}) == capi.KMC_OK


@pytest.mark.parametrize("field", DOUBLES)
def test_create_refuses_non_finite(field):
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert _create_rc(**{field: bad}) == capi.ERR_ARG, (field, bad)


@pytest.mark.parametrize("field", POSITIVE)
def test_create_refuses_non_positive(field):
    for bad in (0.0, -0.0, -1.0, -5e-324):
        assert _create_rc(**{field: bad}) == capi.ERR_ARG, (field, bad)


@pytest.mark.parametrize("field", NON_NEGATIVE)
def test_create_refuses_negative_accepts_zero(field):
    for bad in (-1e-300, -1.0):
        assert _create_rc(**{field: bad}) == capi.ERR_ARG, (field, bad)
    assert _create_rc(**{field: 0.0}) == capi.KMC_OK


def test_create_population_sizes():
    for n_a, n_b, want in [(0, 0, capi.ERR_ARG), (-1, 5, capi.ERR_ARG), (5, -1, capi.ERR_ARG),
                           (1, 0, capi.KMC_OK), (0, 1, capi.KMC_OK), ((1 << 24) + 1, 0, capi.ERR_ARG)]:
        p = params(n_a=n_a, n_b=n_b, **TINY_BOX)
        assert engine.host_check_params(p) == want
        try:
            engine.Simulation(p).close()
            rc = capi.KMC_OK
        except engine.KmcError as e:
            rc = e.code
        assert rc == want, (n_a, n_b)


def test_zero_mobility_and_rates_simulated_like_the_oracle():
    # accepted => simulated like the oracle, at the accepted edge: nothing moves, nothing reacts
    zero = {f: 0.0 for f in NON_NEGATIVE}
    p = params(n_a=30, n_b=10, seed=3, **TINY_BOX, **zero)
    st = engine.host_init_random(p)
    compare_stepwise(p, 20, init_state=st)
