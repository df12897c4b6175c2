"""The on-device bond kinetics recorder (kmc_kinetics.hip; include/kmc.h,
DESIGN.md §15) against its sequential host counterpart (engine.HostKinetics,
which tests/test_kinetics_host.py holds against a plain-Python recorder) fed
with get_state() after each piece of the run.  Every comparison is exact
equality of integers.

Small shape: 150 receptors + 50 ligands (n_a < 256: one padded workgroup),
DENSE rates, seed 23, evolved for 6000 steps, then continued in a new handle
whose dissociation rates are raised to 5e-3 for 600 steps with an update after
every step.  Larger shape: 1200 + 200 in 2200 x 2200 x 250 (several
workgroups, n_a no multiple of 256), started as tests/test_gpu_dynamics.py
starts, 200 steps with an update every 4."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

from _kinetics import ARRAYS, EVENTS
from _kmc import DENSE, REPO, build, capi, engine, params

pytestmark = pytest.mark.gpu

RUN = os.path.join(REPO, "kmc-with-a-diffusion-reaction-algorithm_amd", "lib", "kmc_run")
RESORT = 7
FAST = 5e-3
RATES = dict(diss_rate=FAST, cis_diss_rate=FAST, mono_cis_diss_rate=FAST)


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same(sim, host, out, where):
    """The device recorder's arrays and counters against the host one's."""
    got = sim.kin_arrays()
    for k in ARRAYS:
        g, w = getattr(got, k), getattr(host.arrays, k)
        assert g.dtype == w.dtype
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (where, k, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))
    g, w = out.as_dict(), host.acc.as_dict()
    assert g == w, (where, {k: (g[k], w[k]) for k in w if g[k] != w[k]})


def _same_sample(sim, host, where):
    out, hist = sim.kin_sample()
    want, want_hist = host.sample()
    g, w = out.as_dict(), want.as_dict()
    assert g == w, (where, {k: (g[k], w[k]) for k in w if g[k] != w[k]})
    assert np.array_equal(hist, want_hist), (where, np.argwhere(hist != want_hist)[:4].tolist())
    return w, want_hist


def _recorded_run(p, hs0, steps, every, sample_every):
    """The run with the recorder, every result compared with the host recorder on the way.  Returns (host
    recorder, last sample (out dict, hist), records, final state, clusters, re-sorts launched by the steps)."""
    with _env(KMC_RESORT=str(RESORT)), engine.Simulation(p) as sim:
        sim.set_state(hs0)
        sim.set_timing(("slot_resort",))  # event brackets only: counts the steps' re-sort launches
        sim.kin_begin()
        host = engine.HostKinetics(p, hs0)
        first, _ = sim.kin_sample()
        assert first.as_dict() == host.sample()[0].as_dict()
        recs, last = [], None
        for piece in range(1, steps // every + 1):
            recs.append(sim.step(every))
            out = sim.kin_update()
            host.update(sim.get_state())
            _same(sim, host, out, piece)
            if (piece * every) % sample_every == 0:
                last = _same_sample(sim, host, piece)
        # a second update at the same step: nothing but the count moves
        again = sim.kin_update()
        a, b = again.as_dict(), out.as_dict()
        assert a.pop("n_updates") == b.pop("n_updates") + 1 and a == b
        host.update(sim.get_state())
        _same(sim, host, again, "again")
        assert sim.analysis_ms > 0.0
        clusters = sim.clusters()  # still valid after the recorder's calls
        resorts = sim.kernel_times().get("slot_resort", (0.0, 0))[1]
        return host, last, np.concatenate(recs), sim.get_state(), clusters, resorts


@pytest.fixture(scope="module")
def small_start():
    """(params with the raised dissociation rates, the state after 6000 steps at DENSE rates)."""
    p = params(seed=23, **DENSE)
    assert p.n_a + p.n_b == 200 and p.n_a < 256
    with engine.Simulation(p) as sim:
        sim.set_state(engine.host_init_random(p))
        sim.step(6000)
        hs = sim.get_state()
    kw = dict(DENSE)
    kw.update(RATES)
    return params(seed=23, **kw), hs


def test_small_shape_every_step(small_start):
    p, hs0 = small_start
    steps = 600
    host, (d, hist), _, _, _, resorts = _recorded_run(p, hs0, steps, 1, 100)
    rows = hist.sum(axis=1)
    print("rows", rows.tolist(), {k: d[k] for k in EVENTS})
    # the input exercises every row (asserted on the host side)
    assert rows[0] >= 30, "completed R-L lifetimes"
    assert rows[1] >= 5, "censored R-L bonds ended"
    assert rows[2] >= 15, "mono cis lifetimes"
    assert rows[3] >= 5, "complex cis lifetimes"
    assert rows[4] >= 5, "censored cis bonds ended"
    assert rows[5] >= 30, "rebinding to the same ligand"
    assert (d["origin_step"], d["last_step"], d["n_updates"]) == (hs0.step, hs0.step + steps, steps)
    # slots were permuted between the updates: the re-sorts the steps launched,
    # counted by the engine's own event brackets (one every RESORT steps)
    assert resorts >= 2 and abs(resorts - steps // RESORT) <= 1, resorts


def _large_params(fast):
    kw = dict(DENSE)
    kw.update(box_x=2200.0, box_y=2200.0, box_z=250.0)
    if fast:
        kw.update(RATES)
    return params(seed=7, n_a=1200, n_b=200, **kw)


@pytest.fixture(scope="module")
def large_start():
    """(params with the raised dissociation rates, the evolved state): tests/test_gpu_dynamics.py's recipe."""
    p = _large_params(False)
    assert p.n_a % 256 != 0 and p.n_a > 4 * 256
    with engine.Simulation(p) as sim:
        sim.set_state(engine.host_init_random(p))
        for _ in range(30):
            sim.step(2000)
            hs = sim.get_state()
            nei2, nei3 = hs.a_int[2], hs.a_int[4]
            if hs.counters[1] > 0 and np.any((nei2 == 0) & (nei3 != 0)) and np.any(nei2 == 0):
                break
    assert hs.counters[1] > 0, "no R-L bond after 60000 steps: choose another seed"
    return _large_params(True), hs


LARGE_STEPS, LARGE_EVERY = 200, 4


@pytest.fixture(scope="module")
def large_run(large_start):
    p, hs0 = large_start
    return _recorded_run(p, hs0, LARGE_STEPS, LARGE_EVERY, 40)


def test_large_shape_every_four_steps(large_start, large_run):
    p, hs0 = large_start
    host, (d, hist), _, _, _, resorts = large_run
    print("rows", hist.sum(axis=1).tolist(), {k: d[k] for k in EVENTS})
    assert d["rl_off"] + d["cis_off_mono"] + d["cis_off_cx"] >= 1, "no bond ended: choose another seed"
    assert d["rl_on"] + d["cis_on"] >= 1, "no bond was born: choose another seed"
    assert d["n_updates"] == LARGE_STEPS // LARGE_EVERY and d["last_step"] == hs0.step + LARGE_STEPS
    assert d["occ_rl"] + d["occ_free_receptor"] == p.n_a
    assert resorts >= 2 and abs(resorts - LARGE_STEPS // RESORT) <= 1, resorts


def test_recording_changes_nothing_and_runs_beside_the_tracker(large_start, large_run):
    p, hs0 = large_start
    host, (want_d, want_hist), recs, final, clusters, _ = large_run
    pieces = LARGE_STEPS // LARGE_EVERY
    with _env(KMC_RESORT=str(RESORT)), engine.Simulation(p) as sim:  # neither
        sim.set_state(hs0)
        plain = np.concatenate([sim.step(LARGE_EVERY) for _ in range(pieces)])
        assert np.array_equal(recs, plain)
        assert engine.state_hash(p, final) == engine.state_hash(p, sim.get_state())
        assert final.step == sim.current_step
        row, mem = sim.clusters()
        assert np.array_equal(row, clusters[0]) and np.array_equal(mem, clusters[1])
    with _env(KMC_RESORT=str(RESORT)), engine.Simulation(p) as sim:  # the tracker alone
        sim.set_state(hs0)
        sim.track_begin()
        for _ in range(pieces):
            sim.step(LARGE_EVERY)
            sim.track_update()
        trk_out, trk_vh = sim.track_sample(200.0, 40)
        trk_u, trk_flags = sim.track_displacements()
    with _env(KMC_RESORT=str(RESORT)), engine.Simulation(p) as sim:  # both
        sim.set_state(hs0)
        sim.track_begin()
        sim.kin_begin()
        both = []
        for _ in range(pieces):
            both.append(sim.step(LARGE_EVERY))
            sim.kin_update()
            sim.track_update()
        assert np.array_equal(np.concatenate(both), plain)
        out, vh = sim.track_sample(200.0, 40)
        u, flags = sim.track_displacements()
        assert bytes(out) == bytes(trk_out) and np.array_equal(vh, trk_vh)
        assert np.array_equal(u.view(np.uint64), trk_u.view(np.uint64)) and np.array_equal(flags, trk_flags)
        d, hist = sim.kin_sample()
        assert d.as_dict() == want_d | {"n_updates": pieces} and np.array_equal(hist, want_hist)
        got = sim.kin_arrays()
        assert all(np.array_equal(getattr(got, k), getattr(host.arrays, k)) for k in ARRAYS)
        sim.track_end()  # ending one leaves the other
        assert sim.kin_update().n_updates == pieces + 1
        sim.track_begin()
        sim.kin_end()
        assert sim.track_update().n_updates == 1
        assert engine.state_hash(p, final) == engine.state_hash(p, sim.get_state())


def test_errors(small_start):
    p, hs0 = small_start
    L = engine.load_library()

    def code(f, *a):
        with pytest.raises(engine.KmcError) as e:
            f(*a)
        return e.value.code

    with engine.Simulation(p) as sim:
        # an empty handle
        assert code(sim.kin_begin) == capi.ERR_ARG
        assert code(sim.kin_update) == capi.ERR_ARG
        sim.set_state(hs0)
        # before begin
        assert code(sim.kin_update) == capi.ERR_ARG
        assert code(sim.kin_sample) == capi.ERR_ARG
        assert code(sim.kin_arrays) == capi.ERR_ARG
        sim.kin_begin()
        sim.kin_begin()
        sim.kin_update()
        # null pointers, and the optional ones accepted
        for f in (L.kmc_kin_begin, L.kmc_kin_end):
            assert f(None) == capi.ERR_ARG
        assert L.kmc_kin_update(None, None) == capi.ERR_ARG
        assert L.kmc_kin_sample(None, None, None) == capi.ERR_ARG
        assert L.kmc_kin_get(None, None) == capi.ERR_ARG
        assert L.kmc_kin_sample(sim._h, None, None) == capi.ERR_ARG
        assert L.kmc_kin_get(sim._h, None) == capi.ERR_ARG
        view = capi.KinArrays(p.n_a).view()
        view.bits = None
        assert L.kmc_kin_get(sim._h, view) == capi.ERR_ARG
        assert L.kmc_kin_update(sim._h, None) == capi.KMC_OK  # out is optional
        out = capi.KinOut()
        assert L.kmc_kin_sample(sim._h, out, None) == capi.KMC_OK  # so is hist
        assert out.n_updates == 2 and out.occ_rl + out.occ_free_receptor == p.n_a
        assert out.occ_rl == np.count_nonzero(hs0.a_int[2]) == out.n_rl_censored_alive
        # a new state drops the recorder
        sim.set_state(hs0)
        assert code(sim.kin_update) == capi.ERR_ARG
        assert code(sim.kin_sample) == capi.ERR_ARG
        sim.kin_begin()
        sim.kin_end()
        assert code(sim.kin_update) == capi.ERR_ARG
        sim.kin_end()  # idempotent
        # a decomposed window
        n = p.n_a + p.n_b
        sim.dd_set_state(hs0, np.arange(n), np.ones(n, dtype=np.uint8), np.zeros(5, dtype=np.int32))
        assert code(sim.kin_begin) == capi.ERR_ARG
        assert code(sim.kin_update) == capi.ERR_ARG


def test_run_kinetics(small_start):
    p, hs0 = small_start
    with engine.Simulation(p) as sim:
        sim.set_state(hs0)
        sim.kin_begin()
        recs, out = sim.run_kinetics(130, 30)  # pieces 30 30 30 30 10
        assert len(recs) == 130 and recs["step"][-1] == hs0.step + 130
        assert out.n_updates == 5 and out.last_step == hs0.step + 130 and out.origin_step == hs0.step
        recs, out = sim.run_kinetics(0, 1)
        assert len(recs) == 0 and out is None
        with pytest.raises(ValueError):
            sim.run_kinetics(10, 0)
        # every occupied receptor-step since begin: between 0 and n_a per step
        d, _ = sim.kin_sample()
        assert d.exp_rl + d.exp_free_receptor == 130 * p.n_a


KIN_EVERY = 3


def _run_args(p, steps, out, kin):
    a = [RUN, "--n-a", str(p.n_a), "--n-b", str(p.n_b), "--steps", str(steps), "--out-interval", str(out),
         "--box", repr(p.box_x), repr(p.box_y), repr(p.box_z), "--seed", str(p.seed)]
    for k in ("mono_cis_ass_rate", "cis_ass_rate", "diss_rate", "mono_cis_diss_rate", "cis_diss_rate"):
        a += ["--set", f"{k}={getattr(p, k)!r}"]
    a += ["--state", "state.kmc"]
    return a + (["--kin", str(KIN_EVERY), "kin.dat"] if kin else [])


def _replay_lines(sim, steps):
    """The lines kmc_run --kin writes after `steps` more steps from sim's state."""
    sim.kin_begin()
    sim.run_kinetics(steps, KIN_EVERY)
    out, hist = sim.kin_sample()
    step = sim.current_step
    d = out.as_dict()
    assert d.pop("last_step") == step
    lines = [["kin", step] + list(d.values())]
    lines += [["life", step, r, b, int(hist[r, b])] for r in range(capi.KIN_HISTS) for b in range(capi.KIN_BINS)
              if hist[r, b]]
    return lines


def test_kmc_run_kin(tmp_path):
    # reference size with the raised dissociation rates, two output intervals, the second resumed from the exact
    # state (a new origin); a run without --kin writes the same bond.dat / position.cpt
    assert not build.stale(), "libkmc.so / kmc_run are older than their sources: run __graft_entry__.build()"
    kw = dict(DENSE)
    kw.update(RATES)
    p = params(seed=23, **kw)
    (tmp_path / "kin").mkdir()
    (tmp_path / "plain").mkdir()
    want = []
    for steps in (1000, 2000):
        with engine.Simulation(p) as sim:
            if steps == 1000:
                sim.init_random()
            else:
                sim.load_state(str(tmp_path / "kin" / "state.kmc"))
            assert sim.current_step == steps - 1000
            want += _replay_lines(sim, 1000)
        for d, kin in (("kin", True), ("plain", False)):
            r = subprocess.run(_run_args(p, steps, 1000, kin), cwd=tmp_path / d, capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stderr
        got = [[w[0]] + [int(x) for x in w[1:]] for w in
               (ln.split() for ln in (tmp_path / "kin" / "kin.dat").read_text().splitlines())]
        assert got == want
        for f in ("bond.dat", "position.cpt"):
            assert (tmp_path / "kin" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
    kin = [w for w in want if w[0] == "kin"]
    assert [w[1:4] for w in kin] == [[1000, 0, 334], [2000, 1000, 334]]  # step, origin, updates: 333 pieces of 3 and one of 1
    assert sum(w[4] for w in want if w[0] == "life") > 0
