"""The on-device pair dynamics (kmc_pairdyn.hip; include/kmc.h)
against the brute-force Python reference of tests/_pairdyn.py and the
sequential host twin (engine.HostPd), both fed with get_state() after each
update.  Every comparison is exact equality, but for the cross-check against
kmc_pair_counts, which works in doubles: its bound is counted in the test.

State: test_gpu_lagcorr.py's 1200 receptors + 200 ligands (the fixture recipe
is copied from there), evolved on the GPU until R-L and cis bonds exist, then
continued in a new handle whose dissociation rates are raised to 5e-4.
N = 1400 is not a multiple of 256; the box is 2200 x 2200.  The file's 12 tests
take 10 s on an MI355X."""
import contextlib
import importlib
import os
import subprocess

import numpy as np
import pytest

from _kmc import DENSE, PKG, REPO, build, capi, engine, params
from _lagcorr import min_image
from _pairdyn import RefPd, bins_of, same_arrays, same_sample, sample_tables
from _scale import blocks, evolve, patch_in_large_box, scale_params

pytestmark = pytest.mark.gpu

analysis = importlib.import_module(PKG + ".analysis")

RUN = os.path.join(REPO, "kmc-with-a-diffusion-reaction-algorithm_amd", "lib", "kmc_run")
STEPS, EVERY, R_MAX, NBINS = 300, 5, 150.0, 30
RESORT = 7
FAST = 5e-4
AN_WG_MAX = 2048  # kmc_analysis.hip: workgroups of the grid-stride kernels, k_pd_update and k_pd_walk among them
PD_WAVES = 4      # kmc_pairdyn.hip: cells a workgroup of k_pd_walk takes at once, a wave each
NC_MAX = 2048     # kmc_pairdyn.h PD_NC_MAX: cells per axis


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


def _pd_run(p, hs0, steps=STEPS, every=EVERY, r_max=R_MAX, nbins=NBINS, max_jump=0.0, max_disp=0.0, sample_every=20,
            reference=True, others=False, chunk=None):
    """The run with the recorder: pd_arrays against the twin (and the reference) after every update, the tables against
    the twin (and the reference) at the origin, every sample_every updates and at the end.  Returns (reference or
    None, host twin, last sample, records, final state, clusters, re-sorts the steps launched at each update)."""
    cfg = capi.pd_config(every, nbins, r_max, max_jump, max_disp)
    env = dict(KMC_RESORT=str(RESORT))
    if chunk is not None:
        env["KMC_DEBUG_PD_CHUNK"] = str(chunk)
    with _env(**env), engine.Simulation(p) as sim:
        sim.set_state(hs0)
        sim.set_timing(("slot_resort",))  # event brackets only: counts the steps' re-sort launches
        sim.pd_begin(cfg)
        if others:
            sim.track_begin()
            sim.lag_begin(capi.lag_config(every, 2, 2))
        ref = RefPd(p, hs0, every, nbins, r_max, max_jump, max_disp) if reference else None
        host = engine.HostPd(p, hs0, cfg)

        def compare(n):
            s = sim.pd_sample()
            assert sample_tables(s) == sample_tables(host.sample()), n
            assert (s.ncx, s.ncy) == (host.acc.ncx, host.acc.ncy)
            if ref is not None:
                assert same_sample(s, ref), n
            return s

        U, X0, flags = sim.pd_arrays()
        assert np.array_equal(U, host.arrays.U) and np.array_equal(U, X0) and not flags.any()
        s = compare(0)
        recs, resorts = [], []
        n_updates = steps // every
        for n in range(1, n_updates + 1):
            recs.append(sim.step(every))
            info = sim.pd_update()
            if others:
                sim.track_update()
                sim.lag_update()
            hs = sim.get_state()
            resorts.append(sim.kernel_times().get("slot_resort", (0.0, 0))[1])
            want = host.update(hs)
            assert (info.n_updates, info.n_jumped) == (want.n_updates, want.n_jumped), n
            U, X0, flags = sim.pd_arrays()
            assert np.array_equal(U, host.arrays.U) and np.array_equal(X0, host.arrays.X0), n
            assert np.array_equal(flags, host.arrays.flags), n
            if ref is not None:
                ref.update(hs)
                assert same_arrays(U, X0, flags, ref)
            if n % sample_every == 0 or n == n_updates:
                s = compare(n)
        assert sim.analysis_ms >= 0.0
        clusters = sim.clusters()  # still valid after the recorder's calls
        return ref, host, s, np.concatenate(recs), sim.get_state(), clusters, resorts


@pytest.fixture(scope="module")
def main_run(start):
    p, hs0 = start
    return _pd_run(p, hs0)


def test_recorder_equals_reference_and_input_exercises_it(start, main_run):
    p, hs0 = start
    ref, host, s, _, _, _, resorts = main_run
    assert (s.ncx, s.ncy) == (14, 14) and (s.origin_step, s.last_step, s.n_updates) == (hs0.step, hs0.step + STEPS, 60)
    # the input exercises the layer (asserted on the reference side)
    t = ref.tables()
    assert ref.crossed.any(), "no protein crossed the box edge"
    assert t["seam_a"] > 0 and t["seam_b"] > 0, "no counted pair's minimum image crosses the seam"
    assert all(sum(t["gd"][k]) > 0 for k in range(4)) and all(sum(t["gs"][k]) > 0 for k in range(2))
    assert all(sum(t["n_pairs"][k]) > 0 and sum(t["n_valid"][k]) > 0 for k in range(3)), "a kind without pairs"
    dots = [x for row in t["dot"] for x in row]
    assert min(dots) < 0 < max(dots), "the dot sums have one sign"
    # slots were permuted between the updates (one re-sort every RESORT steps, counted by the engine's own brackets)
    assert resorts[-1] >= 2 and abs(resorts[-1] - STEPS // RESORT) <= 1 and len(set(resorts)) > 2, resorts
    r, gd, gs = analysis.van_hove_distinct(s, p)
    r, cu, valid = analysis.displacement_corr(s)
    assert gd.shape == (4, NBINS) and (gd >= 0).all() and np.abs(cu).max() <= 1.0 and (valid <= 1.0).all()


def test_small_jump_and_displacement_bounds(start):
    p, hs0 = start
    # two updates a step apart: with 1 A an axis nearly every protein is flagged after two updates of five steps
    # (1366 of 1400, no valid BB pair left)
    ref, _, s, *_ = _pd_run(p, hs0, steps=2, every=1, max_jump=1.0, max_disp=50.0, sample_every=1)
    assert (ref.J, ref.F) == (1024, 51200)
    t = ref.tables()
    print("jumped", int(ref.jumped.sum()), "valid pairs by kind", [sum(r) for r in t["n_valid"]],
          "pairs", [sum(r) for r in t["n_pairs"]])
    assert any(v < n for rv, rn in zip(t["n_valid"], t["n_pairs"]) for v, n in zip(rv, rn))
    assert all(sum(t["n_valid"][k]) > 0 for k in range(3)), "a kind without a valid pair"
    assert 0 < int(ref.jumped.sum()) < p.n_a + p.n_b


def test_chunked_path(start, main_run):
    # three points a side at a time: every cell of the 14 x 14 grid (7 proteins a cell) takes several chunks of i
    # and of j, the self cell's triangle among them
    p, hs0 = start
    assert (p.n_a + p.n_b) / (14 * 14) > 2 * 3
    ref, _, s, *_ = _pd_run(p, hs0, chunk=3, sample_every=30, reference=False)
    assert sample_tables(s) == sample_tables(main_run[2]) == {k: v for k, v in main_run[0].tables().items()
                                                              if not k.startswith("seam")}


def test_more_cells_than_one_launch_serves(start):
    # the 1400 proteins re-declared in an 8000 x 8000 box (they stay around the origin, across the fold's seam; in
    # the 2200 box no r_max both fills the AA tables and gives this many cells): r_max = 85 gives 94 x 94 cells,
    # more than the 2048 workgroups of four waves take at once, so the first 644 waves take a second cell
    p0, hs0 = start
    p, hs = patch_in_large_box(p0, hs0, 8000.0, 8000.0, inset=None)
    r_max, nbins = 85.0, 17
    nc = int(8000.0 * 1024) // int(r_max * 1024)
    assert nc == 94 and nc * nc > AN_WG_MAX * PD_WAVES and nc * nc - AN_WG_MAX * PD_WAVES == 644
    ref, _, s, *_ = _pd_run(p, hs, steps=40, r_max=r_max, nbins=nbins, sample_every=4)
    assert (s.ncx, s.ncy) == (nc, nc)
    t = ref.tables()
    assert all(sum(t["gd"][k]) > 0 for k in range(4)) and all(sum(t["n_pairs"][k]) > 0 for k in range(3))
    assert t["seam_a"] > 0 and t["seam_b"] > 0


BIG_X, BIG_Y = 330_000.0, 310_000.0


@pytest.fixture(scope="module")
def patch():
    """test_gpu_layers_scale.py's patch P (3000 + 600 in a 4000 x 3000 box, 10 000 steps): (params, state)."""
    kw = dict(DENSE)
    kw.update(box_x=4000.0, box_y=3000.0, box_z=250.0)
    p0 = params(seed=31, n_a=3000, n_b=600, **kw)
    with engine.Simulation(p0) as sim:
        sim.set_state(engine.host_init_random(p0))
        for _ in range(100):
            sim.step(100)
        return p0, sim.get_state()


@pytest.mark.parametrize("where", ["origin", "corner"])
def test_clamped_grid(patch, where):
    # the patch in the 330 000 x 310 000 box: box / r_max > 2048 on both axes, the grid is clamped and its cells are
    # wider than r_max; untranslated the patch lies across the fold's seam, translated across the box's corner.  The
    # brute-force reference takes all 3600 proteins (2 s), so no subsample is needed.
    p0, hs0 = patch
    p, hs = patch_in_large_box(p0, hs0, BIG_X, BIG_Y, inset=None if where == "origin" else 700.0)
    assert engine.host_validate(p, hs) == capi.KMC_OK
    assert int(BIG_X * 1024) // int(R_MAX * 1024) > NC_MAX and int(BIG_Y * 1024) // int(R_MAX * 1024) > NC_MAX
    assert NC_MAX * NC_MAX > AN_WG_MAX * PD_WAVES
    ref, _, s, *_ = _pd_run(p, hs, steps=8, every=4, sample_every=2)
    assert (s.ncx, s.ncy) == (NC_MAX, NC_MAX)
    t = ref.tables()
    # pairs across both seams remain, asserted on the reference's own coordinates: untranslated the seam is the
    # fold's (coordinate 0, where the grid begins and ends), translated it is the box's (+-box / 2, where the wrapped
    # coordinate of the state jumps); within r_max / 2 of it on either side there are proteins
    for c in range(2):
        x = np.mod(ref.X0[:, c], ref.B[c]) if where == "origin" else ref.X0[:, c] + ref.B[c] // 2
        assert x.min() < 75 * 1024 and x.max() > ref.B[c] - 75 * 1024
    assert (t["seam_a"] > 0 and t["seam_b"] > 0) == (where == "origin")
    assert all(sum(t["gd"][k]) > 0 for k in range(4)) and all(sum(t["n_pairs"][k]) > 0 for k in range(3))


def test_stride_over_the_blocks():
    n_a, n_b = 524_400, 174_800
    n = n_a + n_b
    # 2732 blocks against 2048 workgroups: the first 684 workgroups of k_pd_update take two blocks; the last is ragged
    assert blocks(n) == 2732 > AN_WG_MAX and blocks(n) - AN_WG_MAX == 684 and n % 256 != 0
    p0 = scale_params(n_a, n_b, 5)
    sim0, hs0, _ = evolve(p0, 2000, 10)
    sim0.close()
    p = scale_params(n_a, n_b, 5, fast=True)
    _, host, s, *_ = _pd_run(p, hs0, steps=8, every=4, sample_every=2, reference=False)
    assert s.ncx * s.ncy > AN_WG_MAX * PD_WAVES and int(s.n_updates) == 2
    assert n - n // 100 < int(s.gs.sum()) <= n and all(int(s.gd[k].sum()) > 0 for k in range(4))
    assert all(int(s.n_valid[k].sum()) > 0 for k in range(3)) and int(np.abs(s.dot).sum()) > 0
    assert (host.arrays.U[-256:] != host.arrays.X0[-256:]).any()  # the ragged last block moved


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
    # with a tracker and a lag recorder beside it: the same records, state and tables
    _, _, s2, recs2, final2, clusters2, _ = _pd_run(p, hs0, others=True, reference=False, sample_every=30)
    assert np.array_equal(recs2, want) and engine.state_hash(p, final2) == want_hash
    assert np.array_equal(clusters2[0], clusters[0]) and np.array_equal(clusters2[1], clusters[1])
    assert sample_tables(s2) == sample_tables(s)


def test_cross_check_against_pair_counts_and_the_arrays(start):
    p, hs0 = start
    with engine.Simulation(p) as sim:
        sim.set_state(hs0)
        pc = sim.pair_counts("AA", R_MAX, NBINS)
        sim.pd_begin(capi.pd_config(EVERY, NBINS, R_MAX))
        s0 = sim.pd_sample()
        for _ in range(4):
            sim.step(EVERY)
            sim.pd_update()
        s = sim.pd_sample()
        U, X0, _ = sim.pd_arrays()
    ref = RefPd(p, hs0, EVERY, NBINS, R_MAX)
    # dr = 5 A = 5120 quanta: every integer edge coincides with pair_counts' edge
    assert ref.E == [5120 * m for m in range(NBINS + 1)]
    assert [int(x) for x in s0.gd[0]] == [2 * int(x) for x in s0.n_pairs[0]]
    # pair_counts takes the distance in doubles, the recorder of coordinates rounded to the quantum: each of dx, dy
    # moves by at most one quantum (two roundings of half a quantum), so a pair changes its bin only when moving
    # |dx| and |dy| by up to one quantum each carries it across an edge.  Those pairs are counted here, per edge.
    X = ref.X0[:p.n_a]
    i, j = np.triu_indices(p.n_a, 1)
    dx = np.abs(min_image(X[j, 0] - X[i, 0], ref.B[0]))
    dy = np.abs(min_image(X[j, 1] - X[i, 1], ref.B[1]))
    lo = np.maximum(dx - 1, 0) ** 2 + np.maximum(dy - 1, 0) ** 2
    hi = (dx + 1) ** 2 + (dy + 1) ** 2
    E2 = np.array([e * e for e in ref.E], dtype=np.int64)
    near = np.array([int(np.count_nonzero((lo < e2) & (hi >= e2))) for e2 in E2])
    print("pairs near an edge:", near.tolist(), "counted:", int(pc.sum()), int(s0.gd[0].sum()) // 2)
    for k in range(NBINS):
        assert abs(int(s0.gd[0][k]) - 2 * int(pc[k])) <= 2 * int(near[k] + near[k + 1]), k
    assert abs(int(s0.gd[0].sum()) - 2 * int(pc.sum())) <= 2 * int(near[NBINS])
    assert int(pc.sum()) > 1000
    # the self part is the histogram of the arrays' own folded displacements
    D = [min_image(np.mod(U[:, c], ref.B[c]) - np.mod(X0[:, c], ref.B[c]), ref.B[c]) for c in range(2)]
    k = bins_of(D[0] * D[0] + D[1] * D[1], E2)
    for sp, sel in enumerate((slice(0, p.n_a), slice(p.n_a, None))):
        assert [int(x) for x in s.gs[sp]] == np.bincount(k[sel], minlength=NBINS + 1)[:NBINS].tolist()
    assert int(s.gs[0][0]) < p.n_a  # some receptor left the first bin within 20 steps


def test_errors(start):
    p, hs0 = start
    L = engine.load_library()
    cfg = capi.pd_config(EVERY, NBINS, R_MAX)

    def code(f, *a):
        with pytest.raises(engine.KmcError) as e:
            f(*a)
        return e.value.code

    with engine.Simulation(p) as sim:
        # an empty handle
        assert code(sim.pd_begin, cfg) == capi.ERR_ARG
        assert code(sim.pd_update) == capi.ERR_ARG
        sim.set_state(hs0)
        # before begin
        assert code(sim.pd_update) == capi.ERR_ARG
        assert code(sim.pd_sample) == capi.ERR_ARG
        assert code(sim.pd_arrays) == capi.ERR_ARG
        assert code(sim.run_paired, EVERY, 1) == capi.ERR_ARG
        # the configuration's bounds
        for kw in (dict(every=0), dict(nbins=0), dict(nbins=257), dict(r_max=0.0), dict(r_max=float("nan")),
                   dict(r_max=734.0), dict(r_max=0.001, nbins=256), dict(max_jump=1100.5),
                   dict(max_jump=float("nan")), dict(max_disp=16385.0), dict(max_disp=float("nan"))):
            args = dict(every=EVERY, nbins=NBINS, r_max=R_MAX)
            args.update(kw)
            assert code(sim.pd_begin, capi.pd_config(**args)) == capi.ERR_ARG, kw
        assert L.kmc_pd_begin(sim._h, None) == capi.ERR_ARG
        assert L.kmc_pd_begin(None, None) == capi.ERR_ARG
        sim.pd_begin(capi.pd_config(EVERY, 256, 733.0, 1100.0, 16384.0))  # the bounds themselves
        s = sim.pd_sample()
        assert (s.ncx, s.ncy, s.nbins) == (3, 3, 256)
        sim.pd_begin(cfg)  # a second begin starts over, with another shape
        assert sim.pd_sample().ncx == 14
        # an update off the stride changes nothing
        assert code(sim.pd_update) == capi.ERR_ARG
        sim.step(EVERY - 1)
        assert code(sim.pd_update) == capi.ERR_ARG
        sim.step(2)
        assert code(sim.pd_update) == capi.ERR_ARG
        U, X0, flags = sim.pd_arrays()
        assert sim.pd_sample().n_updates == 0 and np.array_equal(U, X0) and not flags.any()
        # null pointers
        assert L.kmc_pd_sample(sim._h, None, None, None, None) == capi.ERR_ARG
        assert L.kmc_pd_update(None, None) == capi.ERR_ARG
        assert L.kmc_pd_arrays(sim._h, None, None, None) == capi.KMC_OK  # the arrays are optional
        out = capi.PdOut()
        assert L.kmc_pd_sample(sim._h, out, None, None, None) == capi.KMC_OK and out.ncx == 14  # so are the tables
        # on the stride again after a new begin; info is optional
        sim.pd_begin(cfg)
        sim.step(EVERY)
        assert L.kmc_pd_update(sim._h, None) == capi.KMC_OK
        assert sim.pd_sample().n_updates == 1
        # a new state drops the recorder
        sim.set_state(hs0)
        assert code(sim.pd_update) == capi.ERR_ARG
        assert code(sim.pd_sample) == capi.ERR_ARG
        sim.pd_begin(cfg)
        sim.pd_end()
        assert code(sim.pd_update) == capi.ERR_ARG
        sim.pd_end()  # idempotent
        # a decomposed window
        n = p.n_a + p.n_b
        sim.dd_set_state(hs0, np.arange(n), np.ones(n, dtype=np.uint8), np.zeros(5, dtype=np.int32))
        assert code(sim.pd_begin, cfg) == capi.ERR_ARG
        assert code(sim.pd_update) == capi.ERR_ARG


def test_run_paired(start):
    p, hs0 = start
    cfg = capi.pd_config(10, NBINS, R_MAX)
    with engine.Simulation(p) as sim:
        sim.set_state(hs0)
        sim.pd_begin(cfg)
        with pytest.raises(ValueError):
            sim.run_paired(25, 1)
        recs, samples = sim.run_paired(70, 3)
        assert len(recs) == 70 and recs["step"][-1] == hs0.step + 70
        assert [x.lag_steps for x in samples] == [30, 60] and sim.pd_sample().n_updates == 7
    with engine.Simulation(p) as sim:  # the same by single calls
        sim.set_state(hs0)
        sim.pd_begin(cfg)
        for _ in range(6):
            sim.step(10)
            sim.pd_update()
        assert sample_tables(sim.pd_sample()) == sample_tables(samples[1])


def _run_args(p, steps, out, pd):
    a = [RUN, "--n-a", str(p.n_a), "--n-b", str(p.n_b), "--steps", str(steps), "--out-interval", str(out),
         "--box", repr(p.box_x), repr(p.box_y), repr(p.box_z), "--seed", str(p.seed)]
    for k in ("mono_cis_ass_rate", "cis_ass_rate", "diss_rate", "mono_cis_diss_rate", "cis_diss_rate"):
        a += ["--set", f"{k}={getattr(p, k)!r}"]
    a += ["--state", "state.kmc"]
    return a + (["--pd", "30", "11", "150", "15", "pd.dat"] if pd else [])


def _replay_lines(sim, cfg, sample_every, until):
    """The lines kmc_run --pd writes from sim's state until step `until`."""
    sim.pd_begin(cfg)
    lines = []
    while sim.current_step + cfg.every <= until:
        sim.step(cfg.every)
        if sim.pd_update().n_updates % sample_every:
            continue
        s = sim.pd_sample()
        step, o = sim.current_step, s.origin_step
        lines.append(["pd", step, o, s.n_updates, s.every, s.nbins, s.J, s.F, s.BX, s.BY])
        lines += [["gd", step, o, t, k, int(s.gd[t, k])] for t in range(4) for k in range(s.nbins) if int(s.gd[t, k])]
        lines += [["gs", step, o, t, k, int(s.gs[t, k])] for t in range(2) for k in range(s.nbins) if int(s.gs[t, k])]
        lines += [["cu", step, o, t, k] + [int(getattr(s, name)[t, k]) for name in ("n_pairs", "n_valid", "dot", "sq")]
                  for t in range(3) for k in range(s.nbins) if int(s.n_pairs[t, k])]
    if until > sim.current_step:
        sim.step(until - sim.current_step)
    return lines


def test_kmc_run_pd(tmp_path):
    # reference size, two output intervals in the first process, one more in a second that resumes from the exact
    # state (a new origin); a run without --pd writes the same bond.dat / position.cpt
    assert not build.stale(), "libkmc.so / kmc_run are older than their sources: run __graft_entry__.build()"
    p = params(seed=23, **DENSE)
    cfg = capi.pd_config(30, 15, 150.0)
    (tmp_path / "pd").mkdir()
    (tmp_path / "plain").mkdir()
    want = []
    for steps, first in ((2000, 0), (3000, 2000)):
        with engine.Simulation(p) as sim:
            if steps == 2000:
                sim.init_random()
            else:
                sim.load_state(str(tmp_path / "pd" / "state.kmc"))
            assert sim.current_step == first
            want += _replay_lines(sim, cfg, 11, steps)
        for d, pd in (("pd", True), ("plain", False)):
            r = subprocess.run(_run_args(p, steps, 1000, pd), cwd=tmp_path / d, capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stderr
        got = [[w[0]] + [int(x) for x in w[1:]] for w in
               (ln.split() for ln in (tmp_path / "pd" / "pd.dat").read_text().splitlines())]
        assert got == want
        for f in ("bond.dat", "position.cpt"):
            assert (tmp_path / "pd" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
    heads = [w for w in want if w[0] == "pd"]
    # a sample every 330 steps: six in the first process, three since the new origin at 2000
    assert [w[1:4] for w in heads] == [[330 * k, 0, 11 * k] for k in range(1, 7)] + [
        [2000 + 330 * k, 2000, 11 * k] for k in range(1, 4)]
    assert any(w[0] == "cu" and w[7] < 0 for w in want) and any(w[0] == "gd" for w in want)
