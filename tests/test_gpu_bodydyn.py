"""The on-device body dynamics (kmc_bodydyn.hip; include/kmc.h)
against the Python reference of tests/_bodydyn.py and the sequential host twin
(engine.HostBd), both fed with get_state() after each update.  Every comparison
is exact equality.

Main state: test_gpu_geometry.py's 3000 receptors + 600 ligands with the DENSE
rates in a 4000 x 3000 box, evolved 10 000 steps (the recipe is copied from
there), then continued in a new handle whose dissociation rates are raised to
5e-4 so that bodies break within the 300 steps of the run.  N = 3600 is not a
multiple of 256 and not of 64 x 4.  The hand-built cases edit the graph of a
random placement (paths of tests/_bodydyn.py, the brick-wall lattice of
tests/_geometry.py) and set U and the flags through bd_put."""
import contextlib
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from _bodydyn import RefBd, body_tuples, identities, path, row_tuples, same_arrays, same_sample, sample_table
from _geometry import lattice_state, ref_geometry
from _kmc import DENSE, PKG, REPO, build, capi, engine, params
from _scale import blocks, evolve, scale_params

pytestmark = pytest.mark.gpu

analysis = importlib.import_module(PKG + ".analysis")

RUN = os.path.join(REPO, "kmc-with-a-diffusion-reaction-algorithm_amd", "lib", "kmc_run")
STEPS, EVERY, MAX_SIZE = 300, 5, 12
RESORT = 7
FAST = 5e-4
AN_WG_MAX = 2048  # kmc_analysis.hip: workgroups of the grid-stride kernels, k_bd_update, k_bd_reduce, k_bd_finish too
SPAN = 64         # kmc_bodydyn.hip BD_SPAN: list entries a wave of k_bd_reduce takes at a time


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


def _params(fast):
    kw = dict(DENSE)
    kw.update(box_x=4000.0, box_y=3000.0, box_z=250.0)
    if fast:
        kw.update(diss_rate=FAST, cis_diss_rate=FAST, mono_cis_diss_rate=FAST)
    return params(seed=31, n_a=3000, n_b=600, **kw)


def _centred_on_the_corner(p, hs):
    """hs with every rigid body translated by one vector, and wrapped by its bead [1][1] into [-box/2, box/2) (as
    _geometry.lattice_state wraps), so that the centre of the first largest component that does not span lands on
    the box's corner: that body then lies across both seams.  The evolved clusters are small against the box, and
    none of them happens to lie across a seam."""
    geo = ref_geometry(p, hs)
    best = max((c for c in geo["comps"] if not c["span"]), key=lambda c: c["n_r"] + c["n_l"])
    mem = np.flatnonzero(geo["label"] == best["label"])
    box = np.array([p.box_x, p.box_y])
    xy = np.concatenate([np.stack([hs.ra[0], hs.ra[1]], axis=1), np.stack([hs.rb[0], hs.rb[1]], axis=1)])
    centre = (xy[mem] + geo["shift"][mem] * box).mean(axis=0)
    out = hs.copy()
    for arr in (out.ra, out.rb):
        for c in range(2):
            v = arr[c] + (box[c] / 2 - centre[c])
            d = (v - box[c] * np.floor(v / box[c] + 0.5)) - arr[c]
            arr[c::3] += d[None, :]
    assert engine.host_validate(p, out) == capi.KMC_OK
    return out


@pytest.fixture(scope="module")
def start():
    """(params with the raised dissociation rates, the evolved state with a cluster moved onto the box's corner)."""
    p = _params(False)
    with engine.Simulation(p) as sim:
        sim.set_state(engine.host_init_random(p))
        for _ in range(100):
            sim.step(100)
        return _params(True), _centred_on_the_corner(p, sim.get_state())


def _layout(ref, span):
    """(start, size, spans covered) of every body in the member list: bodies by label, members counted."""
    out, at = [], 0
    for r in sorted(ref.members):
        n = len(ref.members[r])
        out.append((at, n, (at + n - 1) // span - at // span + 1))
        at += n
    return out


def _compare(sim, host, ref, hs, n=None):
    """The device's table and list against the twin's and the reference's; returns (sample, table, rows by label)."""
    s = sim.bd_sample()
    bodies = sim.bd_bodies()
    assert sample_table(s) == sample_table(host.sample(hs)), n
    assert np.array_equal(bodies, host.bodies(hs)), n
    if ref is None:
        return s, sample_table(s), None
    t, rows = ref.table(hs)
    assert same_sample(s, ref, t), n
    assert body_tuples(bodies) == row_tuples(rows), n
    assert np.array_equal(bodies[bodies["n_r"] + bodies["n_l"] >= 3], sim.bd_bodies(min_size=3))
    identities(t)
    return s, t, {r["label"]: r for r in rows}


def _bd_run(p, hs0, steps=STEPS, every=EVERY, max_size=MAX_SIZE, max_jump=0.0, max_disp=0.0, sample_every=20,
            reference=True, others=False, span=None):
    """The run with the recorder: bd_arrays against the twin (and the reference) after every update, the table and
    the list against the twin (and the reference) at the origin, every sample_every updates and at the end.  Returns
    (reference or None, host twin, the samples' (sample, table, rows), records, final state, clusters, re-sorts the
    steps launched at each update)."""
    cfg = capi.bd_config(every, max_size, max_jump, max_disp)
    env = dict(KMC_RESORT=str(RESORT))
    if span is not None:
        env["KMC_DEBUG_BD_SPAN"] = str(span)
    with _env(**env), engine.Simulation(p) as sim:
        sim.set_state(hs0)
        sim.set_timing(("slot_resort",))  # event brackets only: counts the steps' re-sort launches
        sim.bd_begin(cfg)
        if others:
            sim.track_begin()
            sim.lag_begin(capi.lag_config(every, 2, 2))
            sim.pd_begin(capi.pd_config(every, 10, 100.0))
        ref = RefBd(p, hs0, every, max_size, max_jump, max_disp) if reference else None
        host = engine.HostBd(p, hs0, cfg)

        def arrays(n):
            U, X0, flags, label, D0 = sim.bd_arrays()
            a = host.arrays
            assert np.array_equal(U, a.U) and np.array_equal(X0, a.X0) and np.array_equal(flags, a.flags), n
            assert np.array_equal(label, a.label) and np.array_equal(D0, a.D0), n
            if ref is not None:
                assert same_arrays(U, X0, flags, label, D0, ref), n
            return U, X0, flags

        U, X0, flags = arrays(0)
        assert np.array_equal(U, X0) and not flags.any()
        got = sim.bd_get()
        assert np.array_equal(got.bits, host.arrays.bits) and np.array_equal(got.links, host.arrays.links)
        samples = [_compare(sim, host, ref, hs0, 0)]
        recs, resorts = [], []
        n_updates = steps // every
        for n in range(1, n_updates + 1):
            recs.append(sim.step(every))
            info = sim.bd_update()
            if others:
                sim.track_update()
                sim.lag_update()
                sim.pd_update()
            hs = sim.get_state()
            resorts.append(sim.kernel_times().get("slot_resort", (0.0, 0))[1])
            want = host.update(hs)
            assert (info.n_updates, info.n_jumped, info.n_changed) == (want.n_updates, want.n_jumped, want.n_changed), n
            if ref is not None:
                assert (info.n_jumped, info.n_changed) == ref.update(hs), n
            arrays(n)
            if n % sample_every == 0 or n == n_updates:
                samples.append(_compare(sim, host, ref, hs, n))
        assert sim.analysis_ms >= 0.0
        got = sim.bd_get()
        assert np.array_equal(got.prev, host.arrays.prev) and np.array_equal(got.links, host.arrays.links)
        clusters = sim.clusters()  # still valid after the recorder's calls
        return ref, host, samples, np.concatenate(recs), sim.get_state(), clusters, resorts


@pytest.fixture(scope="module")
def main_run(start):
    p, hs0 = start
    return _bd_run(p, hs0)


def _coverage(ref, samples):
    """What the run holds, asserted on the reference side."""
    s0, t0, rows0 = samples[0]
    # the origin: everything pristine, nothing moved, cos phi = 1
    for hl in range(2):
        assert t0["n_pristine"][hl] == t0["n_bodies"][hl] == t0["n_valid"][hl] == t0["n_intact"][hl]
        assert t0["c1"][hl] == t0["c2"][hl] == [n << 30 for n in t0["n_rot"][hl]]
        assert not any(t0["m2"][hl]) and not any(t0["phi2"][hl])
    assert sum(t0["n_rot"][0]) > 0 and sum(t0["n_rot"][1]) > 0
    # a body across a seam at the origin: non-zero image shifts in a component that does not span
    seam = [r for r in ref.members if ref.shift[ref.members[r]].any()]
    assert seam and not ref.bits[seam].any(), "no body lies across the box's seam at the origin"
    rows = [r for _, _, rs in samples[1:] for r in rs.values()]
    sizes = lambda keep: sorted({r["n_r"] + r["n_l"] for r in rows if keep(r)})
    assert max(sizes(lambda r: r["is_"] & capi.BD_IS_PRISTINE), default=0) >= 3, "no PRISTINE body of size >= 3"
    assert any(r["status"] == capi.BD_BROKEN for r in rows) and any(r["status"] == capi.BD_GROWN for r in rows)
    phis = [r["phi"] for r in rows if r["phi"] is not None]
    assert min(phis) < 0 < max(phis), "the angles have one sign"
    assert ref.crossed.any(), "no protein crossed the box edge"
    print("sizes pristine", sizes(lambda r: r["is_"] & capi.BD_IS_PRISTINE), "broken",
          sizes(lambda r: r["status"] == capi.BD_BROKEN), "grown", sizes(lambda r: r["status"] == capi.BD_GROWN),
          "rot", len(phis), "seam bodies", len(seam))


def test_recorder_equals_reference_and_input_exercises_it(start, main_run):
    p, hs0 = start
    ref, host, samples, _, _, _, resorts = main_run
    s = samples[-1][0]
    assert (s.origin_step, s.last_step, s.n_updates) == (hs0.step, hs0.step + STEPS, 60) and len(samples) == 4
    _coverage(ref, samples)
    # slots were permuted between the updates (one re-sort every RESORT steps, counted by the engine's own brackets)
    assert resorts[-1] >= 2 and abs(resorts[-1] - STEPS // RESORT) <= 1 and len(set(resorts)) > 2, resorts
    msd, n_valid = analysis.body_msd(s)
    surv = analysis.body_survival(s)
    rot = analysis.body_rotation(s)
    assert msd[0, 1] > 0 and n_valid[0, 1] > 0 and 0 < surv["pristine"][0, 2] <= surv["intact"][0, 2] <= 1
    assert np.nanmax(np.abs(rot["c1"])) <= 1.0
    fit = analysis.body_diffusion([(x.lag_steps, x) for x, _, _ in samples[1:]], p.time_step)
    assert fit["D"][0, 1] > 0 and fit["n_lags"][0, 1] == 3


@pytest.mark.parametrize("span", [8, 3])
def test_short_spans_open_segments(start, main_run, span):
    # shorter spans of list entries: bodies of the evolved state then lie over several spans and their sums come
    # together through the accumulators' atomics; the results are those of the 64-entry spans.  The state's largest
    # body has 11 members: at 8 entries a span its bodies lie over two spans and none over three (the hand-built
    # bodies of test_span_edges_on_hand_built_bodies do), at 3 entries a span they lie over three and more
    p, hs0 = start
    lay = _layout(main_run[0], span)
    assert any(k == 2 for _, _, k in lay) and (span == 8 or any(k >= 3 for _, _, k in lay))
    ref, host, samples, *_ = _bd_run(p, hs0, span=span, sample_every=30, reference=False)
    assert samples[-1][1] == main_run[2][-1][1] and samples[0][1] == main_run[2][0][1]


def test_small_jump_and_displacement_bounds(start):
    p, hs0 = start
    ref, _, samples, *_ = _bd_run(p, hs0, steps=2, every=1, max_jump=1.0, max_disp=50.0, sample_every=1)
    assert (ref.J, ref.F) == (1024, 51200)
    t = samples[-1][1]
    jumped = int(np.count_nonzero(ref.flags & capi.BD_JUMPED))
    print("jumped", jumped, "pristine", [sum(r) for r in t["n_pristine"]], "bodies", [sum(r) for r in t["n_bodies"]])
    assert 0 < jumped < p.n_a + p.n_b
    assert 0 < sum(t["n_pristine"][0]) < sum(t["n_bodies"][0])


def _paths_on_random_placement(sizes, n_a, n_b, box, seed=3):
    """A random placement whose graph is replaced by paths of the given sizes (tests/_bodydyn.py), in this order;
    the receptors and ligands left over stay single."""
    p = params(seed=seed, n_a=n_a, n_b=n_b, box_x=box, box_y=box, box_z=1000.0)
    hs = engine.host_init_random(p)
    hs.a_int[:] = 0
    hs.b_int[:] = 0
    rec, lig = iter(range(n_a)), iter(range(n_b))
    mems = [path(hs, rec, lig, s) for s in sizes]
    assert engine.host_validate(p, hs) == capi.KMC_OK
    return p, hs, mems


def _put_case(p, hs, rng, span=None, max_size=MAX_SIZE, max_disp=0.0, noise=3.0, flag_rate=0.03, far_rate=0.0):
    """bd_begin on hs, then U and the flags set by hand through bd_put: a rigid step of its own for every body, a
    small step of its own for every member, a few flags, a few members past max_disp.  The device against the twin
    and the reference, which get the same arrays.  Returns (reference, table, rows by label)."""
    cfg = capi.bd_config(1, max_size, 0.0, max_disp)
    n = p.n_a + p.n_b
    with _env(**({} if span is None else dict(KMC_DEBUG_BD_SPAN=str(span)))), engine.Simulation(p) as sim:
        sim.set_state(hs)
        sim.bd_begin(cfg)
        ref = RefBd(p, hs, 1, max_size, 0.0, max_disp)
        host = engine.HostBd(p, hs, cfg)
        a = sim.bd_get()
        assert same_arrays(a.U, a.X0, a.flags, a.label, a.D0, ref) and np.array_equal(a.bits, ref.bits)
        u = np.zeros((n, 2), dtype=np.int64)
        for mem in ref.members.values():
            u[mem] = np.round(rng.normal(0.0, 30.0, 2) * 1024.0).astype(np.int64)
        u += np.round(rng.normal(0.0, noise, (n, 2)) * 1024.0).astype(np.int64)
        u[rng.random(n) < far_rate] += ref.F
        flags = (rng.random(n) < flag_rate) * capi.BD_JUMPED | (rng.random(n) < flag_rate) * capi.BD_CHANGED
        for arr in (a, host.arrays, ref):
            arr.U[:] = a.X0 + u
            arr.flags[:] = flags.astype(np.uint8)
        sim.bd_put(a)
        for _ in range(2):  # twice: the accumulators are back at zero after a call
            s, t, rows = _compare(sim, host, ref, hs)
        U, X0, fl, label, D0 = sim.bd_arrays()
        assert same_arrays(U, X0, fl, label, D0, ref)
        return ref, t, rows


def test_span_edges_on_hand_built_bodies():
    # spans of 8 entries; the bodies in list order: 3 + 5 end exactly at the first span's last entry, the 7 begins at
    # the second's first, the 9 lies over two spans, the 20 and the 30 over three and more; N = 301 is no multiple of 8
    sizes = [3, 5, 7, 9, 20, 2, 30, 1, 6, 8, 11, 4]
    p, hs, mems = _paths_on_random_placement(sizes, 201, 100, 2000.0)
    rng = np.random.default_rng(5)
    ref, t, rows = _put_case(p, hs, rng, span=8)
    lay = _layout(ref, 8)
    assert [n for _, n, _ in lay[:len(sizes)]] == sizes and (p.n_a + p.n_b) % 8 == 5
    assert any((at + n) % 8 == 0 and n > 1 for at, n, _ in lay) and any(at % 8 == 0 and n > 1 for at, n, _ in lay)
    assert any(k == 2 for _, _, k in lay) and any(k >= 3 for _, _, k in lay) and any(k == 1 and n > 1 for _, n, k in lay)
    phis = [r["phi"] for r in rows.values() if r["phi"] is not None]
    assert min(phis) < 0 < max(phis) and sum(t["n_valid"][1]) < sum(t["n_bodies"][1]) and sum(t["n_rot"][1]) > 3
    # the same with the spans of 64: the 7 .. 30 cross none or one boundary
    ref, t64, _ = _put_case(p, hs, np.random.default_rng(5))
    assert t64 == t


def test_members_past_max_disp_and_every_body_a_monomer():
    p, hs, _ = _paths_on_random_placement([], 150, 43, 2000.0)
    ref, t, rows = _put_case(p, hs, np.random.default_rng(6), max_disp=50.0, far_rate=0.2, noise=0.0)
    assert t["n_bodies"][0][1] == 150 and t["n_bodies"][1][1] == 43 and len(rows) == 193
    assert 0 < t["n_valid"][0][1] < t["n_pristine"][0][1] < 150 and sum(t["n_rot"][0]) + sum(t["n_rot_skipped"][0]) == 0


@pytest.mark.parametrize("wraps", [False, True])
def test_one_body_holding_every_protein(wraps):
    # the brick-wall lattice: 8192 members in one body, 128 spans; above KMC_BD_ROT_MAX, so no angle is taken
    p, hs = lattice_state(wraps, wraps)
    ref, t, rows = _put_case(p, hs, np.random.default_rng(8), max_size=capi.BD_MAX_SIZE, flag_rate=0.0)
    n = p.n_a + p.n_b
    assert n == 8192 > capi.BD_ROT_MAX and len(rows) == 1 and rows[1]["n_r"] + rows[1]["n_l"] == n
    assert rows[1]["bits"] == (capi.SPAN_X | capi.SPAN_Y if wraps else 0) and rows[1]["is_"] == 3
    assert t["n_rot_skipped"][1][capi.BD_MAX_SIZE] == 1 and t["n_rot"][1][capi.BD_MAX_SIZE] == 0
    assert t["m2"][1][capi.BD_MAX_SIZE] == rows[1]["su_x"] ** 2 + rows[1]["su_y"] ** 2 > 0
    assert bool(ref.shift.any()) == (not wraps)  # the open lattice straddles the box's seams


def test_stride_over_the_blocks():
    n_a, n_b = 524_400, 174_800
    n = n_a + n_b
    # 2732 blocks against 2048 workgroups: the first 684 workgroups of k_bd_update and of k_bd_finish take two blocks,
    # the last is ragged; 10 925 spans against 8192 waves: the first 2733 waves of k_bd_reduce take two spans
    assert blocks(n) == 2732 > AN_WG_MAX and n % 256 != 0 and (n + SPAN - 1) // SPAN > 4 * AN_WG_MAX
    p0 = scale_params(n_a, n_b, 5)
    sim0, hs0, _ = evolve(p0, 2000, 10)
    sim0.close()
    p = scale_params(n_a, n_b, 5, fast=True)
    _, host, samples, *_ = _bd_run(p, hs0, steps=8, every=4, sample_every=2, reference=False)
    s, t, _ = samples[-1]
    assert int(s.n_updates) == 2 and sum(t["n_bodies"][0]) + sum(t["n_bodies"][1]) == s.total_bodies
    assert sum(t["n_rot"][0]) > 0 and sum(t["n_rot"][1]) > 0 and sum(t["n_broken"][1]) > 0
    assert sum(t["sum_size"][0]) + sum(t["sum_size"][1]) == n
    assert (host.arrays.U[-256:] != host.arrays.X0[-256:]).any()  # the ragged last block moved


def test_get_save_load_begin_put_continues_bit_for_bit(start, tmp_path):
    p, hs0 = start
    cfg = capi.bd_config(EVERY, MAX_SIZE)
    path_ = str(tmp_path / "state.kmc")
    with engine.Simulation(p) as a:
        a.set_state(hs0)
        a.bd_begin(cfg)
        for _ in range(3):
            a.step(EVERY)
            a.bd_update()
        kept = a.bd_get()
        a.save_state(path_)
        for _ in range(3):
            a.step(EVERY)
            a.bd_update()
        want = a.bd_get()
    assert kept.flags.any() and (kept.U != kept.X0).any()
    with engine.Simulation(p) as b:
        b.load_state(path_)
        b.bd_begin(cfg)  # the bodies, X0 and D0 of the loaded state; the per-protein state comes from the view
        b.bd_put(kept, b.current_step)
        for _ in range(3):
            b.step(EVERY)
            b.bd_update()
        got = b.bd_get()
        assert b.bd_sample().n_updates == 3
    for name in ("prev", "U", "links", "flags"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert (got.flags != kept.flags).any()


def test_recording_changes_nothing(start, main_run):
    p, hs0 = start
    _, _, samples, recs, final, clusters, _ = main_run
    with _env(KMC_RESORT=str(RESORT)), engine.Simulation(p) as sim:
        sim.set_state(hs0)
        want = np.concatenate([sim.step(EVERY) for _ in range(STEPS // EVERY)])
        assert np.array_equal(recs, want)
        want_hash = engine.state_hash(p, sim.get_state())
        assert engine.state_hash(p, final) == want_hash and final.step == sim.current_step
        row, mem = sim.clusters()
        assert np.array_equal(row, clusters[0]) and np.array_equal(mem, clusters[1])
    # with a tracker, a lag recorder and the pair dynamics beside it: the same records, state and table
    _, _, s2, recs2, final2, clusters2, _ = _bd_run(p, hs0, others=True, reference=False, sample_every=30)
    assert np.array_equal(recs2, want) and engine.state_hash(p, final2) == want_hash
    assert np.array_equal(clusters2[0], clusters[0]) and np.array_equal(clusters2[1], clusters[1])
    assert s2[-1][1] == samples[-1][1]


def test_run_bodies(start):
    p, hs0 = start
    cfg = capi.bd_config(10, MAX_SIZE)
    with engine.Simulation(p) as sim:
        sim.set_state(hs0)
        sim.bd_begin(cfg)
        with pytest.raises(ValueError):
            sim.run_bodies(25, 1)
        recs, samples = sim.run_bodies(70, 3)
        assert len(recs) == 70 and recs["step"][-1] == hs0.step + 70
        assert [x.lag_steps for x in samples] == [30, 60] and sim.bd_sample().n_updates == 7
    with engine.Simulation(p) as sim:  # the same by single calls
        sim.set_state(hs0)
        sim.bd_begin(cfg)
        for _ in range(6):
            sim.step(10)
            sim.bd_update()
        assert sample_table(sim.bd_sample()) == sample_table(samples[1])


def test_errors(start):
    p, hs0 = start
    L = engine.load_library()
    cfg = capi.bd_config(EVERY, MAX_SIZE)

    def code(f, *a):
        with pytest.raises(engine.KmcError) as e:
            f(*a)
        return e.value.code

    with engine.Simulation(p) as sim:
        # an empty handle
        assert code(sim.bd_begin, cfg) == capi.ERR_ARG
        assert code(sim.bd_update) == capi.ERR_ARG
        sim.set_state(hs0)
        # before begin
        for f in (sim.bd_update, sim.bd_sample, sim.bd_bodies, sim.bd_arrays, sim.bd_get):
            assert code(f) == capi.ERR_ARG
        assert code(sim.bd_put, capi.BdArrays(p.n_a + p.n_b)) == capi.ERR_ARG
        assert code(sim.run_bodies, EVERY, 1) == capi.ERR_ARG
        # the configuration's bounds
        for kw in (dict(every=0), dict(max_size=1), dict(max_size=256), dict(max_jump=1500.5),
                   dict(max_jump=float("nan")), dict(max_disp=16385.0), dict(max_disp=float("nan"))):
            args = dict(every=EVERY, max_size=MAX_SIZE)
            args.update(kw)
            assert code(sim.bd_begin, capi.bd_config(**args)) == capi.ERR_ARG, kw
        assert L.kmc_bd_begin(sim._h, None) == capi.ERR_ARG
        assert L.kmc_bd_begin(None, None) == capi.ERR_ARG
        sim.bd_begin(capi.bd_config(EVERY, 255, 1500.0, 16384.0))  # the bounds themselves
        s = sim.bd_sample()
        assert (s.max_size, s.J, s.F) == (255, 1500 * 1024, 1 << 24) and s.n_bodies.shape == (2, 256)
        sim.bd_begin(cfg)  # a second begin starts over, with another shape
        assert sim.bd_sample().max_size == MAX_SIZE
        # an update off the stride changes nothing; a sample and a list off the last update's step
        assert code(sim.bd_update) == capi.ERR_ARG
        sim.step(EVERY - 1)
        assert code(sim.bd_update) == capi.ERR_ARG
        assert code(sim.bd_sample) == capi.ERR_ARG
        assert code(sim.bd_bodies) == capi.ERR_ARG
        sim.step(2)
        assert code(sim.bd_update) == capi.ERR_ARG
        U, X0, flags, _, _ = sim.bd_arrays()
        assert np.array_equal(U, X0) and not flags.any()
        # null pointers
        assert L.kmc_bd_sample(sim._h, None, None) == capi.ERR_ARG
        assert L.kmc_bd_update(None, None) == capi.ERR_ARG
        assert L.kmc_bd_arrays(sim._h, None, None, None, None, None) == capi.KMC_OK  # the arrays are optional
        assert L.kmc_bd_get(sim._h, None) == capi.ERR_ARG and L.kmc_bd_put(sim._h, None, 0) == capi.ERR_ARG
        out = capi.BdOut()
        assert L.kmc_bd_sample(sim._h, out, None) == capi.ERR_ARG  # (the state has moved on)
        # on the stride again after a new begin; info is optional; the table is optional
        sim.bd_begin(cfg)
        sim.step(EVERY)
        assert L.kmc_bd_update(sim._h, None) == capi.KMC_OK
        assert L.kmc_bd_sample(sim._h, out, None) == capi.KMC_OK and out.n_updates == 1 and out.n_bodies > 0
        # the list: min_size, a capacity too small (the true count comes back), no rows
        n = C.c_int64(0)
        assert L.kmc_bd_bodies(sim._h, 0, 10, None, n) == capi.ERR_ARG
        assert L.kmc_bd_bodies(sim._h, 1, 10, None, n) == capi.ERR_ARG
        assert L.kmc_bd_bodies(sim._h, 1, 0, None, n) == capi.ERR_CAPACITY and n.value == out.n_bodies
        assert code(sim.bd_bodies, 1, 5) == capi.ERR_CAPACITY
        assert len(sim.bd_bodies()) == out.n_bodies
        # a view with an unknown flag, a last step in the future
        a = sim.bd_get()
        a.flags[7] = 4
        assert code(sim.bd_put, a) == capi.ERR_ARG
        a.flags[7] = 0
        assert code(sim.bd_put, a, sim.current_step + 1) == capi.ERR_ARG
        sim.bd_put(a, sim.current_step - EVERY)
        sim.bd_update()  # due again: the view's last step
        # a new state drops the recorder
        sim.set_state(hs0)
        assert code(sim.bd_update) == capi.ERR_ARG
        assert code(sim.bd_sample) == capi.ERR_ARG
        sim.bd_begin(cfg)
        sim.bd_end()
        assert code(sim.bd_update) == capi.ERR_ARG
        sim.bd_end()  # idempotent
        # a decomposed window
        n = p.n_a + p.n_b
        sim.dd_set_state(hs0, np.arange(n), np.ones(n, dtype=np.uint8), np.zeros(5, dtype=np.int32))
        assert code(sim.bd_begin, cfg) == capi.ERR_ARG
        assert code(sim.bd_update) == capi.ERR_ARG


def _run_args(p, steps, out, bd):
    a = [RUN, "--n-a", str(p.n_a), "--n-b", str(p.n_b), "--steps", str(steps), "--out-interval", str(out),
         "--box", repr(p.box_x), repr(p.box_y), repr(p.box_z), "--seed", str(p.seed)]
    for k in ("mono_cis_ass_rate", "cis_ass_rate", "diss_rate", "mono_cis_diss_rate", "cis_diss_rate"):
        a += ["--set", f"{k}={getattr(p, k)!r}"]
    a += ["--state", "state.kmc"]
    return a + (["--bd", "30", "11", "6", "bd.dat"] if bd else [])


def _replay_lines(sim, cfg, sample_every, until):
    """The lines kmc_run --bd writes from sim's state until step `until`."""
    sim.bd_begin(cfg)
    lines = []
    while sim.current_step + cfg.every <= until:
        sim.step(cfg.every)
        if sim.bd_update().n_updates % sample_every:
            continue
        s = sim.bd_sample()
        step, o = sim.current_step, s.origin_step
        lines.append(["bd", step, o, s.n_updates, s.every, s.max_size, s.J, s.F, s.BX, s.BY, s.total_bodies])
        lines += [["body", step, o, hl, k] + [int(getattr(s, name)[hl, k]) for name in capi.BD_COUNTS + capi.BD_SUMS]
                  for hl in range(2) for k in range(s.max_size + 1) if int(s.n_bodies[hl, k])]
    if until > sim.current_step:
        sim.step(until - sim.current_step)
    return lines


def test_kmc_run_bd(tmp_path):
    # reference size, two output intervals in the first process, one more in a second that resumes from the exact
    # state (a new origin); a run without --bd writes the same bond.dat / position.cpt
    assert not build.stale(), "libkmc.so / kmc_run are older than their sources: run __graft_entry__.build()"
    p = params(seed=23, **DENSE)
    cfg = capi.bd_config(30, 6)
    (tmp_path / "bd").mkdir()
    (tmp_path / "plain").mkdir()
    want = []
    for steps, first in ((2000, 0), (3000, 2000)):
        with engine.Simulation(p) as sim:
            if steps == 2000:
                sim.init_random()
            else:
                sim.load_state(str(tmp_path / "bd" / "state.kmc"))
            assert sim.current_step == first
            want += _replay_lines(sim, cfg, 11, steps)
        for d, bd in (("bd", True), ("plain", False)):
            r = subprocess.run(_run_args(p, steps, 1000, bd), cwd=tmp_path / d, capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stderr
        got = [[w[0]] + [int(x) for x in w[1:]] for w in
               (ln.split() for ln in (tmp_path / "bd" / "bd.dat").read_text().splitlines())]
        assert got == want
        for f in ("bond.dat", "position.cpt"):
            assert (tmp_path / "bd" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
    heads = [w for w in want if w[0] == "bd"]
    # a sample every 330 steps: six in the first process, three since the new origin at 2000
    assert [w[1:4] for w in heads] == [[330 * k, 0, 11 * k] for k in range(1, 7)] + [
        [2000 + 330 * k, 2000, 11 * k] for k in range(1, 4)]
    assert any(w[0] == "body" and w[3] == 1 and w[4] >= 3 for w in want)
