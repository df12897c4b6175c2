"""The on-device orientation layer (kmc_orient.hip; include/kmc.h, DESIGN.md
§19) against the Python reference of tests/_orient.py and the sequential host
twins (engine.HostRot, engine.host_ligand_pose), fed with get_state() after each
update.  Every comparison is exact equality, but for the float cross-check of
C_1, whose bound is worked out in the test.

State: test_gpu_lagcorr.py's 1200 receptors + 200 ligands (the fixture recipe
is copied from there), evolved on the GPU until R–L and cis bonds exist, then
continued in a new handle whose dissociation rates are raised to 5e-4 so that
bonds break within the recorded window.  N = 1400 is not a multiple of 256, and
N_A = 1200 splits wave 18: its lanes 0..47 hold receptors (one vector) and its
lanes 48..63 ligands (two)."""
import contextlib
import importlib
import os
import subprocess

import numpy as np
import pytest

from _kmc import DENSE, PKG, REPO, build, capi, engine, params
from _orient import RefRot, n_rows, same_arrays, same_info, same_pose, same_sample, sample_tables
from _scale import blocks, evolve, scale_params

pytestmark = pytest.mark.gpu

analysis = importlib.import_module(PKG + ".analysis")

RUN = os.path.join(REPO, "kmc-with-a-diffusion-reaction-algorithm_amd", "lib", "kmc_run")
STEPS, EVERY, LEVELS, SLOTS = 300, 3, 3, 4
RESORT = 7
FAST = 5e-4
AN_WG_MAX = 2048   # kmc_analysis.hip: workgroups of the grid-stride kernels, k_rot_update among them
POSE_WG_MAX = 512  # kmc_orient.hip: workgroups of k_pose
ROT_CHUNK = 64     # kmc_orient.hip: tasks whose partials the LDS holds at a time


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


def _params(fast, **over):
    kw = dict(DENSE)
    kw.update(box_x=2200.0, box_y=2200.0, box_z=250.0)
    if fast:
        kw.update(diss_rate=FAST, cis_diss_rate=FAST, mono_cis_diss_rate=FAST)
    kw.update(over)
    return params(seed=7, n_a=1200, n_b=200, **kw)


@pytest.fixture(scope="module")
def start():
    """(params with the raised dissociation rates, the evolved state)."""
    p = _params(False)
    with engine.Simulation(p) as sim:
        sim.set_state(engine.host_init_random(p))
        for _ in range(30):
            sim.step(2000)
            hs = sim.get_state()
            nei2, nei3 = hs.a_int[2], hs.a_int[4]
            if hs.counters[1] > 0 and np.any((nei2 == 0) & (nei3 != 0)) and np.any(nei2 == 0):
                break
    assert hs.counters[1] > 0, "no R-L bond after 60000 steps: choose another seed"
    return _params(True), hs


def _rot_run(p, hs0, steps=STEPS, every=EVERY, levels=LEVELS, slots=SLOTS, beside=False, rot=True, sample_every=20,
             reference=True, keep_states=False):
    """The run with the recorder: rot_arrays against the twin (and the reference) after every update, the table every
    sample_every updates and at the end.  beside: a lag recorder and a tracker run on the same handle; rot=False: they
    run alone.  Returns a dict."""
    cfg = capi.rot_config(every, levels, slots)
    out = dict(ref=None, host=None, s=None, states=[hs0], arrays=[])
    with _env(KMC_RESORT=str(RESORT)), engine.Simulation(p) as sim:
        sim.set_state(hs0)
        sim.set_timing(("slot_resort",))  # event brackets only: counts the steps' re-sort launches
        if rot:
            sim.rot_begin(cfg)
            ref = out["ref"] = RefRot(p, hs0, every, levels, slots) if reference else None
            host = out["host"] = engine.HostRot(p, hs0, cfg)
            vec, le, chi = sim.rot_arrays()
            assert np.array_equal(vec, host.arrays.vec) and not le.any() and np.array_equal(chi, host.arrays.chi)
        if beside:
            sim.lag_begin(capi.lag_config(every, levels, slots, h=(1,)))
            sim.track_begin()
        recs, resorts = [], []
        n_updates = steps // every
        for n in range(1, n_updates + 1):
            recs.append(sim.step(every))
            if rot:
                info = sim.rot_update()
            if beside:
                sim.lag_update()
                sim.track_update()
            resorts.append(sim.kernel_times().get("slot_resort", (0.0, 0))[1])
            if not rot:
                continue
            hs = sim.get_state()
            want = host.update(hs)
            got = (info.n_updates, info.n_tasks, info.n_events, info.n_flips, info.n_bad)
            assert got == (want.n_updates, want.n_tasks, want.n_events, want.n_flips, want.n_bad), n
            vec, le, chi = sim.rot_arrays()
            assert np.array_equal(vec, host.arrays.vec) and np.array_equal(le, host.arrays.last_event), n
            assert np.array_equal(chi, host.arrays.chi), n
            if ref is not None:
                ref.update(hs)
                assert same_info(info, ref) and same_arrays(vec, le, chi, ref)
            if keep_states:
                out["states"].append(hs)
                out["arrays"].append(le.copy())
            if n % sample_every == 0 or n == n_updates:
                s = out["s"] = sim.rot_sample()
                assert sample_tables(s) == sample_tables(host.sample()), n
                if ref is not None:
                    assert same_sample(s, ref)
        assert sim.analysis_ms >= 0.0
        if beside:
            out["lag"] = sim.lag_sample()
            ts, vh = sim.track_sample(100.0, 16)
            out["track"] = dict(ts.as_dict(), vanhove=vh)
        out["clusters"] = sim.clusters()  # still valid after the recorder's calls
        out.update(recs=np.concatenate(recs), final=sim.get_state(), resorts=resorts)
    return out


@pytest.fixture(scope="module")
def main_run(start):
    p, hs0 = start
    return _rot_run(p, hs0)


def _c1(t, r, c, v, u2):
    return t["s1_clean"][r][c][v] / (t["n_clean"][r][c][v] * u2)


def test_recorder_equals_reference_and_input_exercises_it(start, main_run):
    p, hs0 = start
    ref, s, resorts = main_run["ref"], main_run["s"], main_run["resorts"]
    assert (p.n_a + p.n_b) % 256 != 0 and p.n_a % 64 != 0  # a ragged last block; a wave with both kinds of lanes
    # the input exercises the layer (asserted on the reference side)
    t = ref.tables()
    rows = n_rows(LEVELS, SLOTS)
    assert all(v > 0 for v in t["n_pairs"]) and len(t["n_pairs"]) == rows == 8
    assert all(sum(t["n_all"][r][c][0] for r in range(rows)) > 0 for c in range(5)), "a class without pairs"
    assert all(sum(t["n_all"][r][c][1] for r in range(rows)) > 0 for c in (3, 4)), "no arm pairs"
    unclean = [sum(t["n_all"][r][c][0] - t["n_clean"][r][c][0] for r in range(rows)) for c in range(5)]
    assert any(unclean[:3]) and any(unclean[3:]), unclean
    assert ref.flips_total > 0, "no ligand was reflected"
    # slots were permuted between the updates (one re-sort every RESORT steps, counted by the engine's own brackets)
    assert resorts[-1] >= 2 and abs(resorts[-1] - STEPS // RESORT) <= 1 and len(set(resorts)) > 2, resorts
    # free receptors forget their heading over the window: 0 < C_1(lag 48 steps) < C_1(lag 3 steps) < 1
    ra2 = (p.ra_radius * 1024.0) ** 2
    assert 0.0 < _c1(t, rows - 1, 0, 0, ra2) < _c1(t, 0, 0, 0, ra2) < 1.0
    assert (s.origin_step, s.last_step, s.n_updates) == (hs0.step, hs0.step + STEPS, STEPS // EVERY)
    # every receptor counts once and every ligand twice in every pair filed (no state is bad)
    assert int(s.n_all.sum()) == (p.n_a + 2 * p.n_b) * sum(t["n_pairs"])
    cur = analysis.rot_curves(s, p)
    assert cur["tau"][0] == EVERY * p.time_step and cur["c1"][0, 0, 0] == _c1(t, 0, 0, 0, ra2)
    # network members keep their orientation longer than free units do
    assert cur["c1"][-1, 2, 0] > cur["c1"][-1, 0, 0] and cur["c1"][-1, 4, 0] > cur["c1"][-1, 3, 0]


def test_single_padded_block():
    # N = 200 < 256: one block, padded; N_A = 150 splits wave 2
    p = params(seed=23, **DENSE)
    assert (p.n_a, p.n_b) == (150, 50)
    r = _rot_run(p, engine.host_init_random(p), steps=120, levels=2, slots=2)
    s = r["s"]
    assert s.rows == 3 and all(int(v) > 0 for v in s.n_pairs)
    assert int(s.n_all[0].sum()) == 250 * int(s.n_pairs[0])


def test_more_tasks_than_the_lds_holds():
    # k_rot_update keeps the partials of ROT_CHUNK = 64 tasks in LDS and walks a longer list in chunks; with 16 slots
    # eight levels fire 16 + 7 * 8 = 72 tasks, first at update 16 * 2^7 = 2048.  N = 200, one step an update, the host
    # twin alone (the reference's schedule is compared with the twin's in the host tests).
    p = params(seed=23, **DENSE)
    cfg = capi.rot_config(1, 8, 16)
    hs = engine.host_init_random(p)
    most = 0
    with engine.Simulation(p) as sim:
        sim.set_state(hs)
        sim.rot_begin(cfg)
        host = engine.HostRot(p, hs, cfg)
        for n in range(1, 2049):
            sim.step(1)
            info = sim.rot_update()
            want = host.update(sim.get_state())
            assert (info.n_tasks, info.n_events, info.n_flips) == (want.n_tasks, want.n_events, want.n_flips), n
            most = max(most, int(info.n_tasks))
        assert most == 72 == int(info.n_tasks) > ROT_CHUNK
        vec, le, chi = sim.rot_arrays()
        assert np.array_equal(vec, host.arrays.vec) and np.array_equal(le, host.arrays.last_event)
        s = sim.rot_sample()
    assert sample_tables(s) == sample_tables(host.sample())
    assert s.rows == 72 and all(int(v) > 0 for v in s.n_pairs) and int(s.n_pairs[-1]) == 1


def test_stride_over_the_blocks():
    n_a, n_b = 524_400, 174_800
    n = n_a + n_b
    # k_rot_update: 2732 blocks against 2048 workgroups, the first 684 workgroups take two blocks; the last block is
    # ragged, and N_A is no multiple of 64.  k_pose: 683 blocks of ligands against 512 workgroups
    assert blocks(n) == 2732 > AN_WG_MAX and blocks(n) - AN_WG_MAX == 684 and n % 256 != 0 and n_a % 64 != 0
    assert blocks(n_b) == 683 > POSE_WG_MAX and n_b % 256 != 0
    p0 = scale_params(n_a, n_b, 5)
    sim0, hs0, _ = evolve(p0, 2000, 10)
    sim0.close()
    p = scale_params(n_a, n_b, 5, fast=True)
    r = _rot_run(p, hs0, steps=12, every=4, levels=2, slots=2, sample_every=1, reference=False)
    s = r["s"]
    assert int(s.n_updates) == 3 and [int(v) for v in s.n_pairs] == [3, 2, 0]
    assert int(s.n_all[0].sum()) == 3 * (n_a + 2 * n_b)
    assert int(s.n_clean.sum()) < int(s.n_all.sum()) and int(s.s2_clean.sum()) > 2 ** 64
    assert int(s.n_all[:, 3:, 1].sum()) > 0  # the arms, the ragged last block's among them
    # the pose census on the same state: the device equals the host twin
    with engine.Simulation(p) as sim:
        sim.set_state(r["final"])
        for nz, nc in ((8, 6), (64, 64)):
            hist, out = sim.ligand_pose(nz, nc)
            want, wout = engine.host_ligand_pose(p, r["final"], nz, nc)
            assert np.array_equal(hist, want) and out.as_dict() == wout.as_dict()
            assert int(hist.sum()) == n_b and sum(out.chi_pos) + sum(out.chi_neg) == n_b and int(out.n_bad) == 0
        assert int(hist[1:].sum()) > 0


def test_recording_changes_nothing(start, main_run):
    p, hs0 = start
    s, recs, final, clusters = (main_run[k] for k in ("s", "recs", "final", "clusters"))
    with _env(KMC_RESORT=str(RESORT)), engine.Simulation(p) as sim:
        sim.set_state(hs0)
        want = np.concatenate([sim.step(EVERY) for _ in range(STEPS // EVERY)])
        assert np.array_equal(recs, want)
        want_hash = engine.state_hash(p, sim.get_state())
        assert engine.state_hash(p, final) == want_hash and final.step == sim.current_step
        row, mem = sim.clusters()
        assert np.array_equal(row, clusters[0]) and np.array_equal(mem, clusters[1])
    # a lag recorder and a tracker beside it: the same records, state and table, and theirs are what they are alone
    both = _rot_run(p, hs0, beside=True, reference=False)
    alone = _rot_run(p, hs0, beside=True, rot=False)
    for r in (both, alone):
        assert np.array_equal(r["recs"], want) and engine.state_hash(p, r["final"]) == want_hash
        assert np.array_equal(r["clusters"][0], clusters[0]) and np.array_equal(r["clusters"][1], clusters[1])
    assert sample_tables(both["s"]) == sample_tables(s)
    assert np.array_equal(both["lag"].counts(), alone["lag"].counts()) and int(both["lag"].n_all.sum()) > 0
    assert both["track"].keys() == alone["track"].keys()
    for k in both["track"]:
        assert np.array_equal(np.asarray(both["track"][k]), np.asarray(alone["track"][k])), k


def test_pose_equals_host_and_reference(start, main_run):
    p, hs0 = start
    for hs in (hs0, main_run["final"]):
        with engine.Simulation(p) as sim:
            sim.set_state(hs)
            for nz, nc in ((10, 8), (1, 1), (64, 64), (3, 64)):
                got = sim.ligand_pose(nz, nc)
                assert same_pose(got, p, hs, nz, nc)
                want, wout = engine.host_ligand_pose(p, hs, nz, nc)
                assert np.array_equal(got[0], want) and got[1].as_dict() == wout.as_dict()
                assert sum(got[1].chi_pos) + sum(got[1].chi_neg) == p.n_b == int(got[0].sum())
    hist, out = got
    assert int(hist[0].sum()) > 0 and int(hist[1:].sum()) > 0  # free and bound ligands
    # a bound ligand is laid down: its axis is vertical, the top tilt bin
    assert int(hist[1:, :, :-1].sum()) == 0
    assert min(sum(out.chi_pos), sum(out.chi_neg)) > 0  # the placement holds both hands
    prof = analysis.pose_profile(hist, p)
    assert np.allclose(prof["pdf"].sum(axis=(1, 2))[prof["n"] > 0], 1.0)


def test_errors(start):
    p, hs0 = start
    L = engine.load_library()
    cfg = capi.rot_config(EVERY, LEVELS, SLOTS)

    def code(f, *a):
        with pytest.raises(engine.KmcError) as e:
            f(*a)
        return e.value.code

    with engine.Simulation(p) as sim:
        # an empty handle
        assert code(sim.rot_begin, cfg) == capi.ERR_ARG
        assert code(sim.rot_update) == capi.ERR_ARG
        assert code(sim.ligand_pose, 4, 4) == capi.ERR_ARG
        sim.set_state(hs0)
        # before begin
        assert code(sim.rot_update) == capi.ERR_ARG
        assert code(sim.rot_sample) == capi.ERR_ARG
        assert code(sim.rot_arrays) == capi.ERR_ARG
        assert code(sim.run_rotated, EVERY) == capi.ERR_ARG
        # the configuration's bounds
        for bad in ((EVERY, LEVELS, 3), (EVERY, 21, SLOTS), (0, LEVELS, SLOTS), (EVERY, 0, SLOTS), (EVERY, LEVELS, 18),
                    (EVERY, LEVELS, 0)):
            assert code(sim.rot_begin, capi.rot_config(*bad)) == capi.ERR_ARG, bad
        for nz, nc in ((0, 4), (4, 0), (65, 4), (4, 65)):
            assert code(sim.ligand_pose, nz, nc) == capi.ERR_ARG
        assert L.kmc_rot_begin(sim._h, None) == capi.ERR_ARG
        assert L.kmc_rot_begin(None, None) == capi.ERR_ARG
        assert L.kmc_ligand_pose(sim._h, 4, 4, None, None) == capi.ERR_ARG
        assert L.kmc_ligand_pose(None, 4, 4, None, None) == capi.ERR_ARG
        out = capi.PoseOut()
        assert L.kmc_ligand_pose(sim._h, 4, 4, None, out) == capi.KMC_OK  # the bins are optional
        assert sum(out.chi_pos) + sum(out.chi_neg) == p.n_b
        sim.rot_begin(capi.rot_config(EVERY, 20, 16))  # the bounds themselves
        assert sim.rot_sample().rows == 168
        sim.rot_begin(cfg)  # a second begin starts over, with another shape
        assert sim.rot_sample().rows == 8
        # an update off the stride changes nothing
        assert code(sim.rot_update) == capi.ERR_ARG
        sim.step(EVERY - 1)
        assert code(sim.rot_update) == capi.ERR_ARG
        sim.step(2)
        assert code(sim.rot_update) == capi.ERR_ARG
        s = sim.rot_sample()
        assert s.n_updates == 0 and not any(int(v) for v in s.n_pairs) and not sim.rot_arrays()[1].any()
        # null pointers
        assert L.kmc_rot_sample(sim._h, None, None, None) == capi.ERR_ARG
        assert L.kmc_rot_update(None, None) == capi.ERR_ARG
        assert L.kmc_rot_arrays(sim._h, None, None, None) == capi.KMC_OK  # every array is optional
        out = capi.RotOut()
        assert L.kmc_rot_sample(sim._h, out, None, None) == capi.KMC_OK and out.rows == 8  # so are the tables
        # on the stride again after a new begin; info is optional
        sim.rot_begin(cfg)
        sim.step(EVERY)
        assert L.kmc_rot_update(sim._h, None) == capi.KMC_OK
        assert sim.rot_sample().n_updates == 1
        # a new state drops the recorder
        sim.set_state(hs0)
        assert code(sim.rot_update) == capi.ERR_ARG
        assert code(sim.rot_sample) == capi.ERR_ARG
        sim.rot_begin(cfg)
        sim.rot_end()
        assert code(sim.rot_update) == capi.ERR_ARG
        sim.rot_end()  # idempotent
        # a decomposed window
        n = p.n_a + p.n_b
        sim.dd_set_state(hs0, np.arange(n), np.ones(n, dtype=np.uint8), np.zeros(5, dtype=np.int32))
        assert code(sim.rot_begin, cfg) == capi.ERR_ARG
        assert code(sim.rot_update) == capi.ERR_ARG
        assert code(sim.ligand_pose, 4, 4) == capi.ERR_ARG


def test_run_rotated(start):
    p, hs0 = start
    cfg = capi.rot_config(10, 2, 4)
    with engine.Simulation(p) as sim:
        sim.set_state(hs0)
        sim.rot_begin(cfg)
        with pytest.raises(ValueError):
            sim.run_rotated(25)
        recs, info = sim.run_rotated(70)
        assert len(recs) == 70 and recs["step"][-1] == hs0.step + 70
        assert (info.n_updates, info.n_tasks) == (7, 4)  # n = 7: level 0 alone, j = 1..4
        got = sim.rot_sample()
    with engine.Simulation(p) as sim:  # the same by single calls
        sim.set_state(hs0)
        sim.rot_begin(cfg)
        for _ in range(7):
            sim.step(10)
            sim.rot_update()
        assert sample_tables(sim.rot_sample()) == sample_tables(got)


def _run_args(p, steps, out, layer):
    a = [RUN, "--n-a", str(p.n_a), "--n-b", str(p.n_b), "--steps", str(steps), "--out-interval", str(out),
         "--box", repr(p.box_x), repr(p.box_y), repr(p.box_z), "--seed", str(p.seed)]
    for k in ("mono_cis_ass_rate", "cis_ass_rate", "diss_rate", "mono_cis_diss_rate", "cis_diss_rate"):
        a += ["--set", f"{k}={getattr(p, k)!r}"]
    a += ["--state", "state.kmc"]
    return a + (["--rot", "30", "3", "4", "rot.dat", "--pose", "5", "7", "pose.dat"] if layer else [])


def _replay_lines(sim, cfg, n_intervals, interval):
    """The lines kmc_run --rot and --pose write over n_intervals more output intervals from sim's state."""
    sim.rot_begin(cfg)
    rot, pose = [], []
    due = sim.current_step + cfg.every
    for _ in range(n_intervals):
        # the stride runs on across the output steps: 1000 is no multiple of 30
        end = (sim.current_step // interval + 1) * interval
        while due <= end:
            sim.step(due - sim.current_step)
            sim.rot_update()
            due += cfg.every
        if end > sim.current_step:
            sim.step(end - sim.current_step)
        s = sim.rot_sample()
        step, o = sim.current_step, s.origin_step
        rot.append(["rot", step, o, s.n_updates, s.every, s.levels, s.slots])
        rot += [["cell", step, o, r, int(s.lags[r]), c, v, int(s.n_pairs[r])] +
                [int(getattr(s, k)[r, c, v]) for k in ("n_all", "n_clean", "s1_all", "s1_clean", "s2_clean")]
                for r in range(s.rows) for c in range(capi.LAG_CLASSES) for v in range(capi.ROT_VECS)
                if int(s.n_all[r, c, v])]
        hist, out = sim.ligand_pose(5, 7)
        pose.append(["pose", step, 5, 7, int(out.n_bad)] + [int(x) for x in out.chi_pos] + [int(x) for x in out.chi_neg])
        pose += [["bin", step, k, z, t, int(hist[k, z, t])] for k, z, t in np.ndindex(*hist.shape) if hist[k, z, t]]
    return rot, pose


def test_kmc_run_rot_and_pose(tmp_path):
    # reference size, two output intervals in the first process, one more in a second that resumes from the exact
    # state (a new origin); a run without the options writes the same bond.dat / position.cpt
    assert not build.stale(), "libkmc.so / kmc_run are older than their sources: run __graft_entry__.build()"
    p = params(seed=23, **DENSE)
    cfg = capi.rot_config(30, 3, 4)
    (tmp_path / "rot").mkdir()
    (tmp_path / "plain").mkdir()
    want_rot, want_pose = [], []
    for steps, intervals in ((2000, 2), (3000, 1)):
        with engine.Simulation(p) as sim:
            if steps == 2000:
                sim.init_random()
            else:
                sim.load_state(str(tmp_path / "rot" / "state.kmc"))
            assert sim.current_step == steps - 1000 * intervals
            r, q = _replay_lines(sim, cfg, intervals, 1000)
            want_rot += r
            want_pose += q
        for d, layer in (("rot", True), ("plain", False)):
            r = subprocess.run(_run_args(p, steps, 1000, layer), cwd=tmp_path / d, capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stderr
        for name, want in (("rot.dat", want_rot), ("pose.dat", want_pose)):
            got = [[w[0]] + [int(x) for x in w[1:]] for w in
                   (ln.split() for ln in (tmp_path / "rot" / name).read_text().splitlines())]
            assert got == want, name
        for f in ("bond.dat", "position.cpt"):
            assert (tmp_path / "rot" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
    heads = [w for w in want_rot if w[0] == "rot"]
    assert [w[1:4] for w in heads] == [[1000, 0, 33], [2000, 0, 66], [3000, 2000, 33]]
    assert max(w[-1] for w in want_rot if w[0] == "cell") > 2 ** 64  # a 128-bit sum that needs its high word
    assert sum(w[-1] for w in want_pose if w[0] == "bin" and w[1] == 3000) == p.n_b


def test_c1_cross_check_in_floats(start):
    # C_1 of row 0 per class and vector, recomputed in float64 from the unit vectors of get_state().  The bound is
    # worked out, not chosen: a bead coordinate is rounded to the quantum with an error of at most 2^-11 A, a vector
    # component is the difference of two beads, so it is off by at most e = 2^-10 A, and with both vectors of a pair
    # off by that much per component |d_int / 2^20 - u . u'| <= e (|u|_1 + |u'|_1) + k e^2 (k = 2 components for a
    # heading, 3 for a ligand's vectors).  Both sides divide by the same nominal |u|^2 n, so the normalisation adds
    # nothing; (1 + 2^-40) covers the float sums themselves.
    p, hs0 = start
    e = 2.0 ** -10
    r = _rot_run(p, hs0, steps=15, every=3, levels=1, slots=2, reference=False, keep_states=True)
    s, states, les = r["s"], r["states"], r["arrays"]
    assert [int(v) for v in s.n_pairs] == [5, 4]
    n_a = p.n_a

    def floats(hs):
        def bead(arr, per, j, k):
            q = ((j - 1) * per + (k - 1)) * 3
            return np.stack([arr[q], arr[q + 1], arr[q + 2]], axis=1)
        H = bead(hs.ra, 4, 3, 2) - bead(hs.ra, 4, 3, 1)
        H[:, 2] = 0.0
        o = bead(hs.rb, 2, 1, 1)
        return [np.concatenate([H, bead(hs.rb, 2, 1, 2) - o]), np.concatenate([H * 0.0, bead(hs.rb, 2, 2, 1) - o])]

    from _orient import classes, links
    total = np.zeros((5, 2))
    bound = np.zeros((5, 2))
    count = np.zeros((5, 2))
    for n in range(1, 6):
        now, org = floats(states[n]), floats(states[n - 1])
        cls = classes(links(states[n]), n_a)
        clean = les[n - 1] <= n - 1
        for v in range(2):
            d = (now[v] * org[v]).sum(axis=1)
            b = e * (np.abs(now[v]).sum(axis=1) + np.abs(org[v]).sum(axis=1)) + 3 * e * e
            for c in range(5):
                m = clean & (cls == c)
                total[c, v] += d[m].sum()
                bound[c, v] += b[m].sum()
                count[c, v] += m.sum()
    cur = analysis.rot_curves(s, p)
    u2 = analysis.rot_lengths(p) / 2.0 ** 20
    checked = 0
    for c in range(5):
        for v in range(1 if c < 3 else 2):
            assert count[c, v] == int(s.n_clean[0, c, v]) > 0
            want = total[c, v] / (count[c, v] * u2[c, v])
            tol = bound[c, v] / (count[c, v] * u2[c, v]) * (1.0 + 2.0 ** -40)
            print("class", c, "vector", v, "C1 integer", cur["c1"][0, c, v], "float", want, "bound", tol)
            assert abs(cur["c1"][0, c, v] - want) <= tol
            checked += 1
    assert checked == 7
