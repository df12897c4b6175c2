"""The head of the step off the serial chain (KMC_STEP_CHAIN):
ukind[] / owner[] kept from step to step and reclassified by k_finalize only
where a bond changed, instead of a k_classify launch every step; the BFS of
the candidate ligands in the leading workgroups of k_propose_free, the thread
that registers a complex going on with its parameters; k_cx_check's tests made
by the parameters' thread on the beads it moves itself.  The arrangement must
not change a trajectory: every step's full-state hash and
bond.dat record equal the keyed oracle's, with the knob on (the default) and
off, with and without re-sorts, through an undone chunk, a forced rebuild and
an exact-state resume, on the small dense scenario from its placement (which
forms few complexes: these cases check the classification, the launches and
the host paths).  The complexes' side — the in-kernel BFS, the parameters'
thread's checks, the dissolve, the descriptors, the unit rows of
kmc_get_clusters — is checked from an evolved state of 3000 + 600 proteins
with complexes of one and of several ligands, continued at a dissociation
rate at which hundreds of bonds form and break within the window."""
import os
import re

import numpy as np
import pytest

from _kmc import DENSE, O, engine, params

pytestmark = pytest.mark.gpu

HEAD = ("k_classify", "k_bfs", "k_cx_check")  # launches the new arrangement removes from a plain step


@pytest.fixture(scope="module")
def reference():
    """(params, placement, the oracle's records and per-step hashes), shared and left unchanged."""
    p = params(seed=53, **DENSE)
    o = O.Oracle(p, rng_mode=O.RNG_KEYED)
    o.init_placement()
    st = o.get_state()
    obs, hashes = o.step(1000)
    return p, st, obs, [int(h) for h in hashes]


def _env(monkeypatch, chain, resort):
    if chain is not None:
        monkeypatch.setenv("KMC_STEP_CHAIN", chain)
    if resort is not None:
        monkeypatch.setenv("KMC_RESORT", resort)


@pytest.mark.parametrize("resort", ["0", "7", None])
@pytest.mark.parametrize("chain", [None, "0"])
def test_stepwise_equals_oracle(monkeypatch, reference, chain, resort):
    # KMC_RESORT=0: complexes formed since the start are not in consecutive
    # slots and no re-sort ever runs the full classification; 7: nearly every
    # window has a full-classification step
    _env(monkeypatch, chain, resort)
    p, st, obs_o, hashes = reference
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        for s in range(600):
            rec = sim.step(1)
            h = engine.state_hash(p, sim.get_state())
            assert rec[0] == obs_o[s], f"step {s + 1}: record {rec[0]} != {obs_o[s]}"
            assert h == hashes[s], f"step {s + 1}: hash {h:x} != {hashes[s]:x}"


def test_debug_cross_check_and_counters(monkeypatch, capfd, reference):
    # the full rule evaluated for every slot on every plain step and compared
    # with the kept arrays (a difference latches an error bit: step() raises);
    # the counters show that the incremental path did the work
    _env(monkeypatch, None, "0")
    monkeypatch.setenv("KMC_DEBUG_CLASSIFY", "1")
    monkeypatch.setenv("KMC_DEBUG_COUNTS", "1")
    p, st, obs_o, hashes = reference
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        obs = np.concatenate([sim.step(250) for _ in range(4)])
        assert np.array_equal(obs, obs_o[:1000])
        assert engine.state_hash(p, sim.get_state()) == hashes[999]
    rows = re.findall(r"reclassified (\d+), bfs-registered (\d+), params-heavy (\d+)", capfd.readouterr().err)
    assert len(rows) == 4, rows
    reclassified, registered, heavy = (int(x) for x in rows[-1])
    assert reclassified > 0 and registered > 0 and heavy > 0, rows


def test_clusters_of_the_finished_step(monkeypatch, reference):
    # kmc_get_clusters reports the finished step's units although k_finalize
    # has already reclassified for the next one: equal to the arrangement that
    # classifies at the start of every step, after every step
    p, st, _, _ = reference
    rows = {}
    for chain in (None, "0"):
        _env(monkeypatch, chain, "0")
        if chain is None:
            monkeypatch.delenv("KMC_STEP_CHAIN", raising=False)
        with engine.Simulation(p) as sim:
            sim.set_state(st)
            out = []
            for _ in range(300):
                sim.step(1)
                rl, mem = sim.clusters()
                out.append((rl.tobytes(), mem.tobytes()))
            rows[chain] = out
    assert rows[None] == rows["0"]


def test_list_overflow_replay(monkeypatch, capfd, reference):
    # lists 2^10 times too small: a chunk is undone from the snapshot and
    # replayed, which runs the full classification again
    monkeypatch.setenv("KMC_DEBUG_CAP_SHIFT", "10")
    monkeypatch.setenv("KMC_DEBUG_COUNTS", "1")
    monkeypatch.setenv("KMC_DEBUG_CLASSIFY", "1")
    p, st, obs_o, hashes = reference
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        obs = np.concatenate([sim.step(300), sim.step(300)])
        assert np.array_equal(obs, obs_o[:600])
        assert engine.state_hash(p, sim.get_state()) == hashes[599]
    replays = [int(x) for x in re.findall(r"replays (\d+)", capfd.readouterr().err)]
    assert replays and replays[-1] > 0, "no chunk was undone"


def test_forced_rebuild_without_resort(monkeypatch, capfd):
    # members[] limit lowered: k_finalize latches full rebuilds, which the host
    # does not see — its workgroup applies the rule to every slot itself
    monkeypatch.setenv("KMC_RESORT", "0")
    monkeypatch.setenv("KMC_DEBUG_CX_LIMIT", "64")
    monkeypatch.setenv("KMC_DEBUG_COUNTS", "1")
    monkeypatch.setenv("KMC_DEBUG_CLASSIFY", "1")
    p = params(seed=41, **DENSE)  # (the seed and length at which the threshold is known to fire)
    o = O.Oracle(p)
    o.init_placement()
    with engine.Simulation(p) as sim:
        sim.set_state(o.get_state())
        obs = np.concatenate([sim.step(1000) for _ in range(4)])
        obs_o, _ = o.step(4000, want_hashes=False)
        assert np.array_equal(obs, obs_o)
        assert engine.state_hash(p, sim.get_state()) == o.hash()
    forced = [int(x) for x in re.findall(r"forced rebuilds (\d+)", capfd.readouterr().err)]
    assert forced and forced[-1] > 0, "the members[] threshold never fired"


def test_exact_state_resume(monkeypatch, tmp_path, reference):
    # a state saved in the middle of a run and resumed in a new handle
    monkeypatch.setenv("KMC_DEBUG_CLASSIFY", "1")
    p, st, obs_o, hashes = reference
    path = str(tmp_path / "mid.kmc")
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        sim.step(217)
        sim.save_state(path)
        a = sim.step(200)
        ha = engine.state_hash(p, sim.get_state())
    with engine.Simulation(p) as sim:
        sim.load_state(path)
        b = sim.step(200)
        hb = engine.state_hash(p, sim.get_state())
    assert np.array_equal(a, obs_o[217:417]) and np.array_equal(a, b)
    assert ha == hb == hashes[416]


@pytest.mark.parametrize("chain", [None, "0"])
def test_launch_count(monkeypatch, reference, chain):
    # every kernel bracketed, 50 plain steps after the first: the new
    # arrangement launches none of HEAD, the old one each once per step
    _env(monkeypatch, chain, "0")
    p, st, _, _ = reference
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        sim.step(1)
        sim.set_timing(engine.kernel_names())
        sim.step(50)
        t = sim.kernel_times()
    want = 50 if chain == "0" else 0
    for k in HEAD:
        assert t.get(k, (0.0, 0))[1] == want, (k, t.get(k))
    assert t["k_propose_free"][1] == 50


# ---- from an evolved state with complexes that form, dissolve and lose ligands
BUSY_STEPS = 400


def _busy_params(diss_rate):
    kw = dict(DENSE)
    kw.update(box_x=4000.0, box_y=3000.0, box_z=250.0, diss_rate=diss_rate)
    return params(seed=31, n_a=3000, n_b=600, **kw)


def _rows(p, row_len, members):
    """({ligand: its row}, ligands that are non-root members of a row with several ligands)."""
    off = np.concatenate([[0], np.cumsum(row_len)])
    rows, nonroot = {}, set()
    for b in np.flatnonzero(row_len > 0):
        row = members[off[b]:off[b + 1]]
        rows[int(b)] = row.tobytes()
        ligs = [int(m) for m in row if m > p.n_a]
        if len(ligs) > 1:
            nonroot.update(m - p.n_a - 1 for m in ligs if m != p.n_a + b + 1)
    return rows, nonroot


@pytest.fixture(scope="module")
def busy():
    """The placement evolved 10 000 steps at the dense rates (on the GPU, old arrangement: 16 complexes,
    one with two ligands), then the oracle's records, hashes and unit rows of BUSY_STEPS steps at a
    dissociation rate of 0.002 — computed once, shared, left unchanged."""
    p0 = _busy_params(DENSE["diss_rate"])
    old = os.environ.get("KMC_STEP_CHAIN")
    os.environ["KMC_STEP_CHAIN"] = "0"
    try:
        with engine.Simulation(p0) as sim:
            sim.set_state(engine.host_init_random(p0))
            sim.step(10000)
            st = sim.get_state()
    finally:
        if old is None:
            del os.environ["KMC_STEP_CHAIN"]
        else:
            os.environ["KMC_STEP_CHAIN"] = old
    p = _busy_params(0.002)
    o = O.Oracle(p, rng_mode=O.RNG_KEYED, nbmode=O.NB_CELLS)
    o.set_state(st)
    s0 = o.stats()
    obs, hashes, rows, freed, prev = [], [], [], 0, set()
    for _ in range(BUSY_STEPS):
        rec, h = o.step(1)
        obs.append(rec[0])
        hashes.append(int(h[0]))
        rl, mem = o.clusters()
        r, nonroot = _rows(p, rl, mem)
        freed += sum(1 for b in prev if rl[b] == 1)  # a non-root ligand of a multi-ligand row, free a step later
        prev = nonroot
        rows.append(r)
    s1 = o.stats()
    gained = {k: s1[k] - s0[k] for k in s1}
    # the window does what the tests below rely on (figures of this seed: 290 bonds formed, 301 broken,
    # 539 multi-ligand complex moves, 443 lay-downs, 5 non-root ligands freed)
    assert gained["rl"] > 100 and gained["rld"] > 100 and gained["multi"] > 100 and gained["laydown"] > 100, gained
    assert freed >= 3, freed
    return p, st, obs, hashes, rows


@pytest.mark.parametrize("resort", ["0", None])
@pytest.mark.parametrize("chain", [None, "0"])
def test_busy_complexes_equal_oracle(monkeypatch, capfd, busy, chain, resort):
    # every step: the record, the full-state hash and every unit row of
    # kmc_get_clusters equal the oracle's; with the cross-check on
    _env(monkeypatch, chain, resort)
    monkeypatch.setenv("KMC_DEBUG_CLASSIFY", "1")
    monkeypatch.setenv("KMC_DEBUG_COUNTS", "1")
    p, st, obs_o, hashes, rows_o = busy
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        for s in range(BUSY_STEPS):
            rec = sim.step(1)
            assert rec[0] == obs_o[s], f"step {s + 1}: record {rec[0]} != {obs_o[s]}"
            h = engine.state_hash(p, sim.get_state())
            assert h == hashes[s], f"step {s + 1}: hash {h:x} != {hashes[s]:x}"
            rl, mem = sim.clusters()
            assert _rows(p, rl, mem)[0] == rows_o[s], f"step {s + 1}: unit rows differ from the oracle's"
    out = re.findall(r"reclassified (\d+), bfs-registered (\d+), params-heavy (\d+)", capfd.readouterr().err)
    reclassified, registered, heavy = (int(x) for x in out[-1])
    if chain is None:
        assert reclassified > 500 and registered > 100 and heavy > 100, out[-1]
    else:
        assert (reclassified, registered, heavy) == (0, 0, 0)


def test_full_bfs_every_step_equals_oracle(monkeypatch, busy):
    # KMC_FULL_BFS=1: no complex kept from step to step, every row a BFS from scratch after k_cx_kill — the same
    # records, hashes and unit rows; the launch counts show that the full rebuild ran on every step
    monkeypatch.setenv("KMC_FULL_BFS", "1")
    monkeypatch.setenv("KMC_RESORT", "0")
    p, st, obs_o, hashes, rows_o = busy
    with engine.Simulation(p) as sim:
        sim.set_state(st)
        sim.set_timing(("k_cx_kill",))
        for s in range(BUSY_STEPS):
            rec = sim.step(1)
            assert rec[0] == obs_o[s], f"step {s + 1}: record {rec[0]} != {obs_o[s]}"
            h = engine.state_hash(p, sim.get_state())
            assert h == hashes[s], f"step {s + 1}: hash {h:x} != {hashes[s]:x}"
            rl, mem = sim.clusters()
            assert _rows(p, rl, mem)[0] == rows_o[s], f"step {s + 1}: unit rows differ from the oracle's"
        # (without the knob and without re-sorts: once, for the new state)
        assert sim.kernel_times()["k_cx_kill"][1] >= BUSY_STEPS
