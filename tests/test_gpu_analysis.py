"""The on-device structure analysis (kmc_analysis.hip; include/kmc.h, DESIGN.md
§10) against numpy references on the state read back with get_state():
components and oligomer census (a plain union-find), lateral pair counts (a
brute-force pair loop with the header's expressions).  All results are
integers: every comparison is exact equality."""
import os
import subprocess

import numpy as np
import pytest

from _analysis import chain_state, np_bin, np_census, np_components, np_d2, summary_dict
from _kmc import DENSE, REPO, build, capi, engine, params

pytestmark = pytest.mark.gpu

RUN = os.path.join(REPO, "kmc-with-a-diffusion-reaction-algorithm_amd", "lib", "kmc_run")
STEPS, EVERY = 10000, 100


def _evolved_params():
    # 3000 receptors + 600 ligands, DENSE rates, in a 4000 x 3000 x 250 box (not
    # square on purpose: ncx != ncy).  600 ligands, not more: the placement rules
    # keep a ligand 84.6 A from every receptor domain (main.cpp:358-384), which at
    # this receptor density leaves it the 45 A slab above the receptors, and 129 A
    # from every other ligand — about 800 fit there at all, and the rejection
    # sampler (like the reference's) gives up long before; 600 is DENSE's own
    # ligand density (50 per 1000 x 1000) and is placed in seconds.
    # STEPS: the ligands start in that slab and first have to come down: the CPU
    # oracle has 7 one-ligand complexes after 3000 steps; after 10000 steps (1.3 s
    # on the GPU) this seed has 16 complexes, one of them with two ligands.
    kw = dict(DENSE)
    kw.update(box_x=4000.0, box_y=3000.0, box_z=250.0)
    return params(seed=31, n_a=3000, n_b=600, **kw)


def _check_census(sim, hs, ref_label, max_r, max_l):
    hist, out = sim.census(max_r, max_l)
    ref_hist, ref_sum = np_census(hs, ref_label, max_r, max_l)
    assert np.array_equal(hist, ref_hist)
    assert summary_dict(out) == ref_sum
    assert hist.sum() == out.n_components
    return out


def test_chain_before_any_step():
    # one component of 1800 proteins whose smallest label travels both ways
    # along a receptor–ligand–cis chain; no step taken: kmc_get_clusters refuses
    p, hs = chain_state()
    ref = np_components(hs)
    with engine.Simulation(p) as sim:
        sim.set_state(hs)
        with pytest.raises(engine.KmcError) as e:
            sim.clusters()
        assert e.value.code == capi.ERR_ARG
        label = sim.components()
        assert np.array_equal(label, ref) and np.all(label == 1)
        for max_r, max_l in ((16, 8), (2, 1)):
            out = _check_census(sim, hs, ref, max_r, max_l)
            h_label, h_hist, h_out = engine.host_census(p, hs, max_r, max_l)
            assert np.array_equal(label, h_label) and np.array_equal(sim.census(max_r, max_l)[0], h_hist)
            assert summary_dict(out) == summary_dict(h_out)
        assert (out.n_components, out.n_complexes, out.max_receptors, out.max_ligands) == (1, 1, 1200, 600)
        assert sim.current_step == 0 and sim.get_state().equal(hs)


@pytest.fixture(scope="module")
def evolved():
    """(params, simulation, its state, the state's hash, the run's records, the initial state): STEPS steps
    from the random placement with no analysis call."""
    p = _evolved_params()
    hs0 = engine.host_init_random(p)
    sim = engine.Simulation(p)
    sim.set_state(hs0)
    recs = np.concatenate([sim.step(EVERY) for _ in range(STEPS // EVERY)])
    hs = sim.get_state()
    yield p, sim, hs, engine.state_hash(p, hs), recs, hs0
    sim.close()


def test_evolved_components_and_census(evolved):
    p, sim, hs, h0, _, _ = evolved
    ref = np_components(hs)
    assert hs.counters[0] > 0
    _, ref_sum = np_census(hs, ref, 16, 8)
    nl = np.bincount(ref[p.n_a:] - 1)
    assert nl.max() >= 2, "the evolved state has no component with two ligands"
    assert ref_sum["n_cis_dimers"] > 0
    assert np.array_equal(sim.components(), ref)
    _check_census(sim, hs, ref, 16, 8)
    _check_census(sim, hs, ref, 2, 1)   # clamped into the last row / column
    _check_census(sim, hs, ref, 63, 63)  # 4096 bins: the largest LDS histogram
    with pytest.raises(engine.KmcError) as e:
        sim.census(64, 63)
    assert e.value.code == capi.ERR_ARG
    # read-only: the same state and step after the calls
    assert engine.state_hash(p, sim.get_state()) == h0


def test_analysis_interleaved_changes_nothing(evolved):
    # the run with analysis calls every EVERY steps: the same records and final
    # state as the run without; and each census describes the state the next
    # step's BFS starts from (main.cpp:514-562)
    p, _, hs, h0, recs, hs0 = evolved
    with engine.Simulation(p) as sim:
        sim.set_state(hs0)
        got = []
        for _ in range(STEPS // EVERY):
            _, out = sim.census(8, 4)
            sim.components()
            sim.pair_counts("AB", 300.0, 20)
            got.append(sim.step(EVERY))
            assert got[-1][0]["tot_cluster_num"] == out.n_complexes
            assert got[-1][0]["tot_proteins_in_cluster"] == out.proteins_in_complexes
        assert np.array_equal(np.concatenate(got), recs)
        before = engine.state_hash(p, sim.get_state())
        assert before == h0
        _, out = sim.census(8, 4)
        sim.pair_counts("AA", 300.0, 60)
        assert engine.state_hash(p, sim.get_state()) == before and sim.current_step == STEPS
        row, _ = sim.clusters()  # still the last step's rows
        assert row.sum() > 0
        rec = sim.step(1)[0]
        assert out.n_complexes > 0
        assert rec["tot_cluster_num"] == out.n_complexes
        assert rec["tot_proteins_in_cluster"] == out.proteins_in_complexes


@pytest.fixture(scope="module")
def brute(evolved):
    """Brute-force squared distances of the evolved state, once per species pair."""
    p, _, hs = evolved[:3]
    cache = {}

    def get(which):
        if which not in cache:
            cache[which] = np_d2(hs, p, which)
        return cache[which]

    return get


# r_max 300: 13 x 10 cells; r_max 1000: exactly 4 x 3 cells, the wrap edge (every y neighbour is the whole axis)
@pytest.mark.parametrize("r_max,nbins", [(300.0, 60), (1000.0, 50)])
@pytest.mark.parametrize("which", ["AA", "AB", "BB"])
def test_pair_counts_equal_brute_force(evolved, brute, which, r_max, nbins):
    sim = evolved[1]
    want = np_bin(brute(which), r_max, nbins)
    assert want.sum() > 0
    assert np.array_equal(sim.pair_counts(which, r_max, nbins), want)
    assert np.array_equal(sim.pair_counts(capi.PAIRS[which], r_max, nbins), want)  # repeatable, int selector


@pytest.mark.parametrize("which", ["AA", "AB", "BB"])
def test_pair_counts_chunked_staging(evolved, brute, which, monkeypatch):
    # 7 points staged at a time: every cell takes several chunks on both sides
    p, _, hs = evolved[:3]
    monkeypatch.setenv("KMC_DEBUG_PAIR_CHUNK", "7")
    with engine.Simulation(p) as sim:
        sim.set_state(hs)
        for r_max, nbins in ((300.0, 60), (1000.0, 50)):
            assert np.array_equal(sim.pair_counts(which, r_max, nbins), np_bin(brute(which), r_max, nbins))


def test_bad_arguments(evolved):
    p, sim, hs = evolved[:3]
    L = engine.load_library()

    def code(f, *a):
        with pytest.raises(engine.KmcError) as e:
            f(*a)
        return e.value.code

    assert code(sim.pair_counts, "AA", 1001.0, 50) == capi.ERR_ARG  # floor(3000 / 1001) = 2 cells along y
    assert code(sim.pair_counts, "AA", 0.0, 50) == capi.ERR_ARG
    assert code(sim.pair_counts, "AA", 300.0, 0) == capi.ERR_ARG
    assert code(sim.pair_counts, "AA", 300.0, capi.PAIR_MAX_BINS + 1) == capi.ERR_ARG
    assert code(sim.pair_counts, 3, 300.0, 60) == capi.ERR_ARG
    assert L.kmc_pair_counts(sim._h, 0, 300.0, 60, None) == capi.ERR_ARG
    assert L.kmc_oligomer_census(sim._h, 4, 4, None, None) == capi.ERR_ARG
    assert L.kmc_components(None, None) == capi.ERR_ARG
    assert L.kmc_components(sim._h, None) == capi.KMC_OK  # labels are optional
    # a handle without state, and a decomposed window
    with engine.Simulation(p) as empty:
        assert code(empty.components) == capi.ERR_ARG
        assert code(empty.census, 4, 4) == capi.ERR_ARG
        assert code(empty.pair_counts, "AB", 300.0, 60) == capi.ERR_ARG
        n = p.n_a + p.n_b
        empty.dd_set_state(hs, np.arange(n), np.ones(n, dtype=np.uint8), np.zeros(5, dtype=np.int32))
        assert code(empty.components) == capi.ERR_ARG
        assert code(empty.census, 4, 4) == capi.ERR_ARG
        assert code(empty.pair_counts, "AB", 300.0, 60) == capi.ERR_ARG


def _run_args(p, steps, out):
    a = [RUN, "--n-a", str(p.n_a), "--n-b", str(p.n_b), "--steps", str(steps), "--out-interval", str(out),
         "--box", repr(p.box_x), repr(p.box_y), repr(p.box_z), "--seed", str(p.seed)]
    for k in ("mono_cis_ass_rate", "cis_ass_rate", "diss_rate", "mono_cis_diss_rate", "cis_diss_rate"):
        a += ["--set", f"{k}={getattr(p, k)!r}"]
    return a + ["--state", "state.kmc", "--census", "census.dat", "--rdf", "AB", "300", "30", "rdf.dat"]


def test_kmc_run_census_and_rdf(tmp_path):
    # two output intervals at reference size (the second resumed from the exact
    # state: the files are appended to); each interval's lines equal the Python
    # calls on the state file written at that step
    assert not build.stale(), "libkmc.so / kmc_run are older than their sources: run __graft_entry__.build()"
    p = params(seed=23, **DENSE)
    want_c, want_r = [], []
    for steps in (1000, 2000):
        r = subprocess.run(_run_args(p, steps, 1000), cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        with engine.Simulation(p) as sim:
            sim.load_state(str(tmp_path / "state.kmc"))
            assert sim.current_step == steps
            hist, _ = sim.census(63, 63)
            counts = sim.pair_counts("AB", 300.0, 30)
        want_c += [[steps, i, j, int(hist[i, j])] for i in range(64) for j in range(64) if hist[i, j]]
        want_r += [[steps, k, int(c)] for k, c in enumerate(counts)]
        got_c = [[int(x) for x in ln.split()] for ln in (tmp_path / "census.dat").read_text().splitlines()]
        got_r = [[int(x) for x in ln.split()] for ln in (tmp_path / "rdf.dat").read_text().splitlines()]
        assert got_c == want_c
        assert got_r == want_r
    assert sum(c[3] for c in want_c if c[0] == 2000) > 0 and sum(c[2] for c in want_r) > 0
