"""The on-device lag correlator (kmc_lagcorr.hip; include/kmc.h)
against the Python reference of tests/_lagcorr.py and the sequential host twin
(engine.HostLag), both fed with get_state() after each update.  Every
comparison is exact equality, but for the cross-check against the tracker,
which has another definition and floats: its bound is worked out in the test.

State: test_gpu_dynamics.py's 1200 receptors + 200 ligands (the fixture recipe
is copied from there), evolved on the GPU until R–L and cis bonds exist, then
continued in a new handle whose dissociation rates are raised to 5e-4 so that
bonds break within the recorded window.  N = 1400 is not a multiple of 256."""
import contextlib
import importlib
import os
import subprocess

import numpy as np
import pytest

from _dynamics import Tracker
from _kmc import DENSE, PKG, REPO, build, capi, engine, params
from _lagcorr import RefLag, n_rows, same_arrays, same_sample, sample_tables
from _scale import blocks, evolve, scale_params

pytestmark = pytest.mark.gpu

analysis = importlib.import_module(PKG + ".analysis")

RUN = os.path.join(REPO, "kmc-with-a-diffusion-reaction-algorithm_amd", "lib", "kmc_run")
STEPS, EVERY, LEVELS, SLOTS, H = 300, 5, 3, 4, (1, 3)
RESORT = 7
FAST = 5e-4
AN_WG_MAX = 2048  # kmc_analysis.hip: workgroups of the grid-stride kernels, k_lag_update among them


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


def _lag_run(p, hs0, steps=STEPS, every=EVERY, levels=LEVELS, slots=SLOTS, max_jump=0.0, max_disp=0.0, h=H,
             tracker=False, sample_every=20, reference=True):
    """The run with the recorder: lag_arrays against the reference after every update, the table against the host
    twin and the reference every sample_every updates and at the end.  Returns (reference or None, host twin, last
    sample, records, final state, clusters, re-sorts the steps launched at each update)."""
    cfg = capi.lag_config(every, levels, slots, max_jump, max_disp, h)
    with _env(KMC_RESORT=str(RESORT)), engine.Simulation(p) as sim:
        sim.set_state(hs0)
        sim.set_timing(("slot_resort",))  # event brackets only: counts the steps' re-sort launches
        sim.lag_begin(cfg)
        if tracker:
            sim.track_begin()
        ref = RefLag(p, hs0, every, levels, slots, max_jump, max_disp, h) if reference else None
        host = engine.HostLag(p, hs0, cfg)
        U, le = sim.lag_arrays()
        assert np.array_equal(U, host.arrays.U) and not le.any()
        recs, resorts, s = [], [], None
        n_updates = steps // every
        for n in range(1, n_updates + 1):
            recs.append(sim.step(every))
            info = sim.lag_update()
            if tracker:
                sim.track_update()
            hs = sim.get_state()
            resorts.append(sim.kernel_times().get("slot_resort", (0.0, 0))[1])
            want = host.update(hs)
            assert (info.n_updates, info.n_tasks, info.n_events) == (want.n_updates, want.n_tasks, want.n_events), n
            U, le = sim.lag_arrays()
            assert np.array_equal(U, host.arrays.U) and np.array_equal(le, host.arrays.last_event), n
            if ref is not None:
                ref.update(hs)
                assert same_arrays(U, le, ref)
            if n % sample_every == 0 or n == n_updates:
                s = sim.lag_sample()
                assert sample_tables(s) == sample_tables(host.sample()), n
                if ref is not None:
                    assert same_sample(s, ref)
        assert sim.analysis_ms >= 0.0
        clusters = sim.clusters()  # still valid after the recorder's calls
        return ref, host, s, np.concatenate(recs), sim.get_state(), clusters, resorts


@pytest.fixture(scope="module")
def main_run(start):
    p, hs0 = start
    return _lag_run(p, hs0)


def test_recorder_equals_reference_and_input_exercises_it(start, main_run):
    p, hs0 = start
    ref, host, s, _, _, _, resorts = main_run
    # the input exercises the layer (asserted on the reference side)
    t = ref.tables()
    assert all(v > 0 for v in t["n_pairs"]) and len(t["n_pairs"]) == n_rows(LEVELS, SLOTS) == 8
    assert any(t["n_clean"][r][c] < t["n_all"][r][c] for r in range(8) for c in range(5)), "every pair is clean"
    assert ref.crossed.any(), "no protein crossed the box edge"
    assert all(sum(t["n_all"][r][c] for r in range(8)) > 0 for c in range(5)), "a class without members"
    # slots were permuted between the updates (one re-sort every RESORT steps, counted by the engine's own brackets)
    assert resorts[-1] >= 2 and abs(resorts[-1] - STEPS // RESORT) <= 1 and len(set(resorts)) > 2, resorts
    assert any(sum(cell) != 0 for row in t["fs"] for cell in row)
    assert (s.origin_step, s.last_step, s.n_updates) == (hs0.step, hs0.step + STEPS, STEPS // EVERY)
    # every protein counts once in every pair filed
    assert int(s.n_all.sum() + s.n_far.sum()) == (p.n_a + p.n_b) * sum(t["n_pairs"])
    cur = analysis.lag_curves(s, p.time_step)
    assert cur["tau"][0] == EVERY * p.time_step and (cur["msd"][:, 0] > 0.0).all()
    assert np.all(np.diff(cur["msd"][:, 0]) > 0.0), "the free receptors' MSD does not grow with the lag"


def test_far_pairs(start):
    p, hs0 = start
    ref, _, s, *_ = _lag_run(p, hs0, max_disp=50.0)
    assert ref.F == 51200
    far = [sum(ref.t["n_far"][r]) for r in range(8)]
    assert far[-1] > 0 and far[-2] > 0, far
    assert far[-1] * ref.n_pairs[0] > far[0] * ref.n_pairs[-1], "the longest lag holds no larger share of far pairs"
    assert [int(v) for v in s.n_far.sum(axis=1)] == far


def test_small_jump_threshold(start):
    p, hs0 = start
    ref, _, s, *_ = _lag_run(p, hs0, steps=120, max_jump=1.0)
    n_all, n_clean = int(s.n_all.sum()), int(s.n_clean.sum())
    assert n_all - n_clean > n_all // 2, (n_all, n_clean)


def test_single_padded_block():
    # N = 200 < 256: one block, padded
    p = params(seed=23, **DENSE)
    assert p.n_a + p.n_b == 200
    ref, _, s, *_ = _lag_run(p, engine.host_init_random(p), steps=120, levels=2, slots=2)
    assert s.rows == 3 and all(int(v) > 0 for v in s.n_pairs)
    assert int(s.n_all[0].sum() + s.n_far[0].sum()) == 200 * int(s.n_pairs[0])


def test_more_tasks_than_the_lds_holds():
    # k_lag_update keeps the partials of 64 tasks in LDS and walks a longer list in chunks; with 16 slots eight
    # levels fire 16 + 7 * 8 = 72 tasks, first at update 16 * 2^7 = 2048 (level 7: t = 16 >= j).  N = 200, one step
    # an update, the host twin alone (the reference's schedule is compared with the twin's in the host tests).
    p = params(seed=23, **DENSE)
    cfg = capi.lag_config(1, 8, 16, h=(1,))
    hs = engine.host_init_random(p)
    most = 0
    with engine.Simulation(p) as sim:
        sim.set_state(hs)
        sim.lag_begin(cfg)
        host = engine.HostLag(p, hs, cfg)
        for n in range(1, 2049):
            sim.step(1)
            info = sim.lag_update()
            want = host.update(sim.get_state())
            assert (info.n_tasks, info.n_events) == (want.n_tasks, want.n_events), n
            most = max(most, int(info.n_tasks))
        assert most == 72 == int(info.n_tasks) > 64
        U, le = sim.lag_arrays()
        assert np.array_equal(U, host.arrays.U) and np.array_equal(le, host.arrays.last_event)
        s = sim.lag_sample()
    assert sample_tables(s) == sample_tables(host.sample())
    assert s.rows == 72 and all(int(v) > 0 for v in s.n_pairs) and int(s.n_pairs[-1]) == 1


def test_stride_over_the_blocks():
    n_a, n_b = 524_400, 174_800
    n = n_a + n_b
    # 2732 blocks against 2048 workgroups: the first 684 workgroups take two blocks; the last block is ragged
    assert blocks(n) == 2732 > AN_WG_MAX and blocks(n) - AN_WG_MAX == 684 and n % 256 != 0
    p0 = scale_params(n_a, n_b, 5)
    sim0, hs0, _ = evolve(p0, 2000, 10)
    sim0.close()
    p = scale_params(n_a, n_b, 5, fast=True)
    _, host, s, *_ = _lag_run(p, hs0, steps=12, every=4, levels=2, slots=2, h=(1,), sample_every=1, reference=False)
    assert int(s.n_updates) == 3 and [int(v) for v in s.n_pairs] == [3, 2, 0]
    assert int(s.n_all[0].sum() + s.n_far[0].sum()) == 3 * n
    assert int(s.n_clean.sum()) < int(s.n_all.sum()) and int(s.m4_clean.sum()) > 0
    assert int(s.n_all[:, 3:].sum()) > 0  # the ligands, the ragged last block's among them


def test_recording_changes_nothing(start, main_run):
    p, hs0 = start
    _, _, s, recs, final, clusters, _ = main_run
    with _env(KMC_RESORT=str(RESORT)), engine.Simulation(p) as sim:
        sim.set_state(hs0)
        want = np.concatenate([sim.step(EVERY) for _ in range(STEPS // EVERY)])
        assert np.array_equal(recs, want)
        want_hash = engine.state_hash(p, sim.get_state())
        assert engine.state_hash(p, final) == want_hash and final.step == sim.current_step
        row, mem = sim.clusters()
        assert np.array_equal(row, clusters[0]) and np.array_equal(mem, clusters[1])
    # with a tracker beside it: the same records, state and table
    _, _, s2, recs2, final2, clusters2, _ = _lag_run(p, hs0, tracker=True, reference=False)
    assert np.array_equal(recs2, want) and engine.state_hash(p, final2) == want_hash
    assert np.array_equal(clusters2[0], clusters[0]) and np.array_equal(clusters2[1], clusters[1])
    assert sample_tables(s2) == sample_tables(s)


def test_errors(start):
    p, hs0 = start
    L = engine.load_library()
    cfg = capi.lag_config(EVERY, LEVELS, SLOTS, h=H)

    def code(f, *a):
        with pytest.raises(engine.KmcError) as e:
            f(*a)
        return e.value.code

    with engine.Simulation(p) as sim:
        # an empty handle
        assert code(sim.lag_begin, cfg) == capi.ERR_ARG
        assert code(sim.lag_update) == capi.ERR_ARG
        sim.set_state(hs0)
        # before begin
        assert code(sim.lag_update) == capi.ERR_ARG
        assert code(sim.lag_sample) == capi.ERR_ARG
        assert code(sim.lag_arrays) == capi.ERR_ARG
        assert code(sim.run_lagged, EVERY) == capi.ERR_ARG
        # the configuration's bounds
        for kw in (dict(slots=3), dict(levels=21), dict(every=0), dict(h=(65,)), dict(max_jump=1100.5),
                   dict(max_jump=float("nan")), dict(max_disp=16385.0), dict(max_disp=float("nan"))):
            args = dict(every=EVERY, levels=LEVELS, slots=SLOTS, h=H)
            args.update(kw)
            assert code(sim.lag_begin, capi.lag_config(**args)) == capi.ERR_ARG, kw
        assert L.kmc_lag_begin(sim._h, None) == capi.ERR_ARG
        assert L.kmc_lag_begin(None, None) == capi.ERR_ARG
        sim.lag_begin(capi.lag_config(EVERY, 20, 16, 1100.0, 16384.0, (64, 1, 64, 1)))  # the bounds themselves
        assert sim.lag_sample().rows == 168
        sim.lag_begin(cfg)  # a second begin starts over, with another shape
        assert sim.lag_sample().rows == 8
        # an update off the stride changes nothing
        assert code(sim.lag_update) == capi.ERR_ARG
        sim.step(EVERY - 1)
        assert code(sim.lag_update) == capi.ERR_ARG
        sim.step(2)
        assert code(sim.lag_update) == capi.ERR_ARG
        s = sim.lag_sample()
        assert s.n_updates == 0 and not any(int(v) for v in s.n_pairs) and not sim.lag_arrays()[1].any()
        # null pointers
        assert L.kmc_lag_sample(sim._h, None, None, None) == capi.ERR_ARG
        assert L.kmc_lag_update(None, None) == capi.ERR_ARG
        assert L.kmc_lag_arrays(sim._h, None, None) == capi.KMC_OK  # both arrays are optional
        out = capi.LagOut()
        assert L.kmc_lag_sample(sim._h, out, None, None) == capi.KMC_OK and out.rows == 8  # so are the tables
        # on the stride again after a new begin; info is optional
        sim.lag_begin(cfg)
        sim.step(EVERY)
        assert L.kmc_lag_update(sim._h, None) == capi.KMC_OK
        assert sim.lag_sample().n_updates == 1
        # a new state drops the recorder
        sim.set_state(hs0)
        assert code(sim.lag_update) == capi.ERR_ARG
        assert code(sim.lag_sample) == capi.ERR_ARG
        sim.lag_begin(cfg)
        sim.lag_end()
        assert code(sim.lag_update) == capi.ERR_ARG
        sim.lag_end()  # idempotent
        # a decomposed window
        n = p.n_a + p.n_b
        sim.dd_set_state(hs0, np.arange(n), np.ones(n, dtype=np.uint8), np.zeros(5, dtype=np.int32))
        assert code(sim.lag_begin, cfg) == capi.ERR_ARG
        assert code(sim.lag_update) == capi.ERR_ARG


def test_run_lagged(start):
    p, hs0 = start
    cfg = capi.lag_config(10, 2, 4, h=(2,))
    with engine.Simulation(p) as sim:
        sim.set_state(hs0)
        sim.lag_begin(cfg)
        with pytest.raises(ValueError):
            sim.run_lagged(25)
        recs, info = sim.run_lagged(70)
        assert len(recs) == 70 and recs["step"][-1] == hs0.step + 70
        assert (info.n_updates, info.n_tasks) == (7, 4)  # n = 7: level 0 alone, j = 1..4
        got = sim.lag_sample()
    with engine.Simulation(p) as sim:  # the same by single calls
        sim.set_state(hs0)
        sim.lag_begin(cfg)
        for _ in range(7):
            sim.step(10)
            sim.lag_update()
        assert sample_tables(sim.lag_sample()) == sample_tables(got)


def _run_args(p, steps, out, lag):
    a = [RUN, "--n-a", str(p.n_a), "--n-b", str(p.n_b), "--steps", str(steps), "--out-interval", str(out),
         "--box", repr(p.box_x), repr(p.box_y), repr(p.box_z), "--seed", str(p.seed)]
    for k in ("mono_cis_ass_rate", "cis_ass_rate", "diss_rate", "mono_cis_diss_rate", "cis_diss_rate"):
        a += ["--set", f"{k}={getattr(p, k)!r}"]
    a += ["--state", "state.kmc"]
    return a + (["--lag", "30", "3", "4", "lag.dat"] if lag else [])


def _replay_lines(sim, cfg, n_intervals, interval):
    """The lines kmc_run --lag writes over n_intervals more output intervals from sim's state."""
    sim.lag_begin(cfg)
    lines = []
    due = sim.current_step + cfg.every
    for _ in range(n_intervals):
        # the stride runs on across the output steps: 1000 is no multiple of 30
        end = (sim.current_step // interval + 1) * interval
        while due <= end:
            sim.step(due - sim.current_step)
            sim.lag_update()
            due += cfg.every
        if end > sim.current_step:
            sim.step(end - sim.current_step)
        s = sim.lag_sample()
        step, o = sim.current_step, s.origin_step
        lines.append(["lag", step, o, s.n_updates, s.every, s.levels, s.slots, s.J, s.F, s.BX, s.BY])
        lines += [["cell", step, o, r, int(s.lags[r]), c, int(s.n_pairs[r])] +
                  [int(getattr(s, k)[r, c]) for k in ("n_all", "n_clean", "n_far", "m2_all", "m2_clean", "m4_clean")]
                  for r in range(s.rows) for c in range(capi.LAG_CLASSES) if int(s.n_all[r, c]) or int(s.n_far[r, c])]
    return lines


def test_kmc_run_lag(tmp_path):
    # reference size, two output intervals in the first process, one more in a second that resumes from the exact
    # state (a new origin); a run without --lag writes the same bond.dat / position.cpt
    assert not build.stale(), "libkmc.so / kmc_run are older than their sources: run __graft_entry__.build()"
    p = params(seed=23, **DENSE)
    cfg = capi.lag_config(30, 3, 4)
    (tmp_path / "lag").mkdir()
    (tmp_path / "plain").mkdir()
    want = []
    for steps, intervals in ((2000, 2), (3000, 1)):
        with engine.Simulation(p) as sim:
            if steps == 2000:
                sim.init_random()
            else:
                sim.load_state(str(tmp_path / "lag" / "state.kmc"))
            assert sim.current_step == steps - 1000 * intervals
            want += _replay_lines(sim, cfg, intervals, 1000)
        for d, lag in (("lag", True), ("plain", False)):
            r = subprocess.run(_run_args(p, steps, 1000, lag), cwd=tmp_path / d, capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stderr
        got = [[w[0]] + [int(x) for x in w[1:]] for w in
               (ln.split() for ln in (tmp_path / "lag" / "lag.dat").read_text().splitlines())]
        assert got == want
        for f in ("bond.dat", "position.cpt"):
            assert (tmp_path / "lag" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
    heads = [w for w in want if w[0] == "lag"]
    assert [w[1:4] for w in heads] == [[1000, 0, 33], [2000, 0, 66], [3000, 2000, 33]]
    assert max(w[-1] for w in want if w[0] == "cell") > 2 ** 64  # a 128-bit sum that needs its high word


def test_cross_check_against_the_tracker(start):
    p, hs0 = start
    e = 3.0 * 2.0 ** -11  # A: two quantised endpoints and the quantised box
    with engine.Simulation(p) as sim:
        sim.set_state(hs0)
        sim.lag_begin(capi.lag_config(EVERY, 1, 2))
        sim.track_begin()
        trk = Tracker(p, hs0)
        U0, _ = sim.lag_arrays()
        sim.step(EVERY)
        sim.lag_update()
        sim.track_update()
        trk.update(sim.get_state())
        s = sim.lag_sample()
        U, _ = sim.lag_arrays()
    u = trk.u  # the numpy tracker's, [N, 2] float64
    assert int(s.n_far.sum()) == 0 and [int(v) for v in s.n_pairs] == [1, 0]
    assert int(s.n_all[0].sum()) == p.n_a + p.n_b
    # the two minimum images chose the same image: another one would differ by a box
    assert np.abs((U - U0) / 1024.0 - u).max() <= e * (1.0 + 2.0 ** -40)
    bound = float(np.sum(2.0 * e * (np.abs(u[:, 0]) + np.abs(u[:, 1])) + 2.0 * e * e)) * (1.0 + 2.0 ** -40)
    got = int(s.m2_all[0].sum()) / 2.0 ** 20
    want = float(np.sum(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]))
    print("sum u^2: integer", got, "tracker", want, "difference", got - want, "bound", bound)
    assert abs(got - want) <= bound
