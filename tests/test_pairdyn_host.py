"""Host side of the pair dynamics: the sequential counterpart
kmc_host_pd_* (engine.HostPd, which sorts by cell) against the brute-force
Python reference of tests/_pairdyn.py (which knows no cells) on hand-made
states, with the values that can be worked out by hand asserted as such;
analysis.van_hove_distinct / displacement_corr and the addition of samples
through analysis.reduce_counts.  Every comparison of the two recorders is exact
equality.  No device needed."""
import ctypes as C
import importlib

import numpy as np
import pytest

from _kmc import PKG, capi, engine, params
from _pairdyn import RefPd, edges, same_arrays, same_sample, sample_tables

analysis = importlib.import_module(PKG + ".analysis")

BOX = dict(box_x=1000.0, box_y=800.0)   # BX = 1 024 000, BY = 819 200
Q = 1.0 / 1024.0                         # the coordinate quantum, A


def _state(p, step, xy):
    """A host state that holds only what the recorder reads: xy[N, 2] of bead [1][1]."""
    hs = capi.HostState(p.n_a, p.n_b)
    xy = np.asarray(xy, dtype=np.float64)
    hs.ra[0], hs.ra[1] = xy[:p.n_a, 0], xy[:p.n_a, 1]
    hs.rb[0], hs.rb[1] = xy[p.n_a:, 0], xy[p.n_a:, 1]
    hs.step = step
    return hs


def _both(p, hs, every, nbins, r_max, max_jump=0.0, max_disp=0.0):
    cfg = capi.pd_config(every, nbins, r_max, max_jump, max_disp)
    return engine.HostPd(p, hs, cfg), RefPd(p, hs, every, nbins, r_max, max_jump, max_disp)


def _advance(host, ref, hs):
    info = host.update(hs)
    ref.update(hs)
    assert (info.n_updates, info.n_jumped) == (ref.n, int(ref.jumped.sum()))
    assert same_arrays(host.arrays.U, host.arrays.X0, host.arrays.flags, ref)


def _same(host, ref):
    s = host.sample()
    assert same_sample(s, ref)
    return s, ref.tables()


def test_edges_and_a_pair_exactly_on_one():
    # E[m] = m * 10 240; receptors 0-1 are E[3] apart along x (bin 3), 0-2 one quantum less along y (bin 2)
    p = params(n_a=3, n_b=0, **BOX)
    assert edges(100.0, 10) == [m * 10240 for m in range(11)]
    xy = np.array([[100.0, 100.0], [130.0, 100.0], [100.0, 130.0 - Q]])
    host, ref = _both(p, _state(p, 0, xy), 1, 10, 100.0)
    s, t = _same(host, ref)
    # 1-2: 30720^2 + 30719^2 = 1 887 375 361 >= E[4]^2 = 1 677 721 600, < E[5]^2: bin 4
    assert t["n_pairs"][0] == [0, 0, 1, 1, 1, 0, 0, 0, 0, 0] and t["gd"][0] == [0, 0, 2, 2, 2, 0, 0, 0, 0, 0]
    assert t["gs"][0][0] == 3 and t["n_valid"] == t["n_pairs"]
    # the same pair one quantum inside and exactly on r_max = E[nbins]: counted, not counted
    xy = np.array([[100.0, 100.0], [200.0 - Q, 100.0], [100.0, 200.0]])
    host, ref = _both(p, _state(p, 0, xy), 1, 10, 100.0)
    s, t = _same(host, ref)
    assert t["n_pairs"][0] == [0] * 9 + [1]


def test_seam_both_directions_both_axes():
    # 0-1 straddle the x seam, 2-3 the y seam (part B at the origin); then 0 and 2 cross it forwards, 1 and 3
    # backwards (part A: origin against now, the pair's image and the self part's)
    p = params(n_a=2, n_b=2, **BOX)
    xy0 = np.array([[999.5, 100.0], [0.5, 100.0], [500.0, 799.5], [500.0, 0.5]])
    move = np.array([[2.0, 0.0], [-2.0, 0.0], [0.0, 2.0], [0.0, -2.0]])
    box = np.array([p.box_x, p.box_y])
    host, ref = _both(p, _state(p, 0, xy0), 3, 8, 40.0)
    s, t = _same(host, ref)
    assert t["seam_a"] == 4 and t["seam_b"] == 2
    assert t["n_pairs"][0][0] == 1 and t["n_pairs"][2][0] == 1  # AA and BB, 1 A apart
    xy = xy0
    for k in range(1, 4):
        xy = np.mod(xy + move, box)
        _advance(host, ref, _state(p, 3 * k, xy))
        s, t = _same(host, ref)
    assert ref.crossed.all() and t["seam_a"] == 4
    # every protein moved 6 A: self bin 1 (5 A wide); the partners moved apart to 13 A: bin 2
    assert t["gs"] == [[0, 2, 0, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0, 0, 0]]
    assert t["gd"][0][1] == 2 and t["gd"][3][1] == 2  # now 7 A from where the partner was
    # the displacements are opposite: dot = -(6144^2), sq = 2 * 6144^2 in both cells, C_u = -1
    assert t["dot"][0][0] == t["dot"][2][0] == -6144 ** 2 and t["sq"][0][0] == 2 * 6144 ** 2
    r, cu, valid = analysis.displacement_corr(s)
    assert cu[0, 0] == -1.0 and cu[2, 0] == -1.0 and cu[1].tolist() == [0.0] * 8 and valid[0, 0] == 1.0


def test_smallest_grid_random_walk():
    # r_max = 260: E[nbins] = 266 240, ncx = floor(1 024 000 / 266 240) = 3, ncy = floor(819 200 / 266 240) = 3; the
    # steps of ~40 A carry proteins into neighbour cells, so i == j is found there too
    p = params(n_a=37, n_b=20, **BOX)
    rng = np.random.default_rng(3)
    n, box = 57, np.array([p.box_x, p.box_y])
    xy = np.floor(rng.random((n, 2)) * box * 1024.0) * Q
    host, ref = _both(p, _state(p, 0, xy), 2, 7, 260.0)
    assert (host.acc.ncx, host.acc.ncy) == (3, 3)
    s, t = _same(host, ref)
    # at the origin: gd[AB] == gd[BA], the self part is all in bin 0, every pair valid with dot = sq = 0
    assert t["gd"][1] == t["gd"][2] and t["gs"][0][0] == 37 and t["gs"][1][0] == 20
    assert [2 * x for x in t["n_pairs"][0]] == t["gd"][0] and t["n_pairs"][1] == t["gd"][1]
    assert t["n_valid"] == t["n_pairs"] and not any(any(row) for k in ("dot", "sq") for row in t[k])
    moved_cell = False
    for k in range(1, 7):
        new = np.mod(xy + np.round(rng.normal(0.0, 40.0, (n, 2)) * 1024.0) * Q, box)
        cell = lambda a: np.floor(np.mod(a, box) * 3 / box)
        moved_cell |= bool((cell(new) != cell(xy)).any())
        xy = new
        _advance(host, ref, _state(p, 2 * k, xy))
        s, t = _same(host, ref)
    assert moved_cell and ref.crossed.any() and t["seam_a"] > 0 and t["seam_b"] > 0
    # the folded self part is the true displacement's while |u| < box / 2
    u = host.arrays.U - host.arrays.X0
    assert np.abs(u).max() < 819200 // 2
    assert sum(t["gs"][0]) + sum(t["gs"][1]) == int(np.count_nonzero((u * u).sum(axis=1) < ref.E[-1] ** 2)) >= n - 3
    assert all(sum(t["gd"][k]) > 0 for k in range(4)) and all(sum(t["n_pairs"][k]) > 0 for k in range(3))
    assert any(x < 0 for row in t["dot"] for x in row) and any(x > 0 for row in t["dot"] for x in row)


def test_self_part_in_a_neighbour_cell():
    # one protein 1 A left of the cell boundary x = 1000 / 3 steps 2 A to the right: its i == j pair is found in the
    # neighbour cell; the second protein keeps the species table apart
    p = params(n_a=1, n_b=1, **BOX)
    b = 1024000 // 3 + 1  # the first folded coordinate of cell 1: floor(b * 3 / BX) = 1
    assert (b - 1) * 3 // 1024000 == 0 and b * 3 // 1024000 == 1
    xy0 = np.array([[(b - 1024) * Q, 400.0], [700.0, 100.0]])
    host, ref = _both(p, _state(p, 0, xy0), 1, 10, 260.0)
    _advance(host, ref, _state(p, 1, xy0 + np.array([[2.0, 0.0], [0.0, 0.0]])))
    s, t = _same(host, ref)
    assert t["gs"] == [[1] + [0] * 9, [1] + [0] * 9] and (host.acc.ncx, host.acc.ncy) == (3, 3)


def test_jump_exactly_at_the_threshold():
    # J = 51 200: protein 0 steps exactly J (jumped, for good), protein 1 one quantum less; 2 stays
    p = params(n_a=3, n_b=0, **BOX)
    xy0 = np.array([[100.0, 100.0], [100.0, 120.0], [100.0, 140.0]])
    host, ref = _both(p, _state(p, 0, xy0), 1, 10, 100.0, max_jump=50.0)
    assert host.acc.J == 51200
    _advance(host, ref, _state(p, 1, xy0 + np.array([[50.0, 0.0], [50.0 - Q, 0.0], [0.0, 0.0]])))
    assert list(host.arrays.flags) == [capi.PD_JUMPED, 0, 0]
    _advance(host, ref, _state(p, 2, xy0 + np.array([[51.0, 0.0], [51.0, 0.0], [0.0, 0.0]])))
    assert list(host.arrays.flags) == [capi.PD_JUMPED, 0, 0]  # sticky
    s, t = _same(host, ref)
    assert sum(t["n_pairs"][0]) == 3 and sum(t["n_valid"][0]) == 1  # only 1-2
    assert sum(t["gs"][0]) == 3  # part A takes the jumped protein as it is


def test_displacement_at_the_bound():
    # F = 2^24 (max_disp = 16 384 A) in a 30 000 A box, two steps of 8192 A (J = 15 000 A): u = +-(F - 1) is valid and
    # gives the largest terms, u = F on one axis is not
    p = params(n_a=3, n_b=2, box_x=30000.0, box_y=30000.0)
    F = 1 << 24
    xy0 = np.array([[10.0, 10.0], [20.0, 10.0], [10.0, 20.0], [20.0, 20.0], [15.0, 15.0]])
    sign = np.array([[1, 1], [-1, -1], [1, 0], [1, -1], [-1, 1]], dtype=np.float64)
    last = np.array([8192.0 - Q] * 2 + [8192.0] + [8192.0 - Q] * 2)[:, None]
    box = np.array([p.box_x, p.box_y])
    host, ref = _both(p, _state(p, 0, xy0), 1, 4, 20.0, max_jump=15000.0, max_disp=16384.0)
    assert host.acc.F == F and host.acc.J == 15000 * 1024
    xy = np.mod(xy0 + sign * 8192.0, box)
    _advance(host, ref, _state(p, 1, xy))
    xy = np.mod(xy + sign * last, box)
    _advance(host, ref, _state(p, 2, xy))
    u = host.arrays.U - host.arrays.X0
    assert u.tolist() == [[F - 1, F - 1], [1 - F, 1 - F], [F, 0], [F - 1, 1 - F], [1 - F, F - 1]]
    assert not host.arrays.flags.any() and ref.valid().tolist() == [True, True, False, True, True]
    s, t = _same(host, ref)
    assert sum(sum(r) for r in t["n_pairs"]) == 10 and sum(sum(r) for r in t["n_valid"]) == 6
    # AA 0-1: dot = -2 (F - 1)^2, sq = 4 (F - 1)^2, the bounds of include/kmc.h
    k01 = 1  # 10 A apart, bins 5 A wide: E[2] = 10 240 <= d
    assert t["dot"][0][2] == -2 * (F - 1) ** 2 and t["sq"][0][2] == 4 * (F - 1) ** 2 and k01
    assert -2 ** 49 < t["dot"][0][2] and t["sq"][0][2] < 2 ** 50
    # BB 3-4: opposite too; AB: 0-3 and 1-4 orthogonal ... the cells' signs are mixed
    assert any(x < 0 for row in t["dot"] for x in row) and all(x >= 0 for row in t["sq"] for x in row)
    # the sums of two such samples need the limbs: add them through reduce_counts
    both = s.from_counts(analysis.reduce_counts(s.counts() + s.counts()))
    assert sample_tables(both)["dot"][0][2] == -4 * (F - 1) ** 2 and sample_tables(both)["sq"][0][2] == 8 * (F - 1) ** 2


@pytest.mark.parametrize("nbins", [1, capi.PD_MAX_BINS])
def test_one_bin_and_the_most_bins(nbins):
    p = params(n_a=30, n_b=30, **BOX)
    rng = np.random.default_rng(nbins)
    box = np.array([p.box_x, p.box_y])
    xy = np.floor(rng.random((60, 2)) * box * 1024.0) * Q
    host, ref = _both(p, _state(p, 0, xy), 1, nbins, 200.0)
    xy = np.mod(xy + np.round(rng.normal(0.0, 10.0, (60, 2)) * 1024.0) * Q, box)
    _advance(host, ref, _state(p, 1, xy))
    s, t = _same(host, ref)
    assert len(t["gd"][0]) == nbins and sum(sum(r) for r in t["n_pairs"]) > 0
    assert np.array_equal(s.from_counts(s.counts()).counts(), s.counts())


def test_two_recorders_add_through_reduce_counts():
    p = params(n_a=25, n_b=15, **BOX)
    rng = np.random.default_rng(11)
    box = np.array([p.box_x, p.box_y])
    samples = []
    for rec in range(2):
        xy = np.floor(rng.random((40, 2)) * box * 1024.0) * Q
        host, ref = _both(p, _state(p, 10 * rec, xy), 5, 6, 250.0)
        for k in (1, 2):
            xy = np.mod(xy + np.round(rng.normal(0.0, 30.0, (40, 2)) * 1024.0) * Q, box)
            _advance(host, ref, _state(p, 10 * rec + 5 * k, xy))
        samples.append(_same(host, ref)[0])
    assert samples[0].lag_steps == samples[1].lag_steps == 10
    total = samples[0].from_counts(analysis.reduce_counts(samples[0].counts() + samples[1].counts()))
    a, b, c = (sample_tables(x) for x in (samples[0], samples[1], total))
    for name in a:
        assert c[name] == [[x + y for x, y in zip(ra, rb)] for ra, rb in zip(a[name], b[name])], name
    assert any(x < 0 for row in c["dot"] for x in row)


def test_analysis_on_a_hand_written_table():
    p = params(n_a=4, n_b=2, box_x=100.0, box_y=50.0)
    out = capi.PdOut()
    out.cfg = capi.pd_config(1, 2, 10.0)
    gd = np.array([[6, 0], [0, 4], [0, 4], [1, 0]], dtype=np.int64)
    gs = np.array([[3, 1], [0, 1]], dtype=np.int64)
    cu = np.zeros((3, 2), dtype=capi.PD_CELL_DTYPE)
    cu["n_pairs"] = [[3, 0], [0, 4], [1, 0]]
    cu["n_valid"] = [[3, 0], [0, 2], [0, 0]]
    cu["dot"]["lo"][0, 0], cu["sq"]["lo"][0, 0] = 50, 100          # rigid co-translation: C_u = 1
    cu["dot"]["lo"][1, 1], cu["dot"]["hi"][1, 1] = 2 ** 64 - 30, -1  # -30
    cu["sq"]["lo"][1, 1] = 120
    s = capi.PdSample(out, gd, gs, cu)
    r, g, self_part = analysis.van_hove_distinct(s, p)
    assert r.tolist() == [2.5, 7.5]
    area = np.pi * np.array([25.0, 75.0]) / 5000.0
    assert np.allclose(g[0], [6 / (4 * 3 * area[0]), 0.0], rtol=1e-15)
    assert np.allclose(g[1], [0.0, 4 / (4 * 2 * area[1])], rtol=1e-15) and np.array_equal(g[1], g[2])
    assert np.allclose(g[3], [1 / (2 * 1 * area[0]), 0.0], rtol=1e-15)
    assert self_part.tolist() == [[0.75, 0.25], [0.0, 0.5]]
    r, c, valid = analysis.displacement_corr(s)
    assert c.tolist() == [[1.0, 0.0], [0.0, -0.5], [0.0, 0.0]]
    assert valid.tolist() == [[1.0, 0.0], [0.0, 0.5], [0.0, 0.0]]


def test_every_err_arg():
    p = params(n_a=3, n_b=2, **BOX)
    hs = _state(p, 0, np.arange(10.0).reshape(5, 2) * 50.0)
    good = dict(every=1, nbins=10, r_max=100.0, max_jump=0.0, max_disp=0.0)
    for kw in (dict(every=0), dict(nbins=0), dict(nbins=capi.PD_MAX_BINS + 1), dict(r_max=0.0), dict(r_max=-1.0),
               dict(r_max=float("nan")), dict(r_max=float("inf")),
               dict(r_max=267.0),                    # floor(819 200 / 273 408) = 2 cells along y
               dict(r_max=0.001, nbins=256),         # every edge rounds to 0: not increasing
               dict(r_max=0.25, nbins=256),          # dr = 1 quantum: 0, 1, 2, ... increases -> good, see below
               dict(max_jump=400.5), dict(max_jump=float("nan")), dict(max_disp=16385.0),
               dict(max_disp=float("nan"))):
        args = dict(good)
        args.update(kw)
        cfg = capi.pd_config(**args)
        if kw == dict(r_max=0.25, nbins=256):
            assert engine.HostPd(p, hs, cfg).acc.ncx == 2048  # 1 024 000 / 256 = 4000 cells, capped
            continue
        with pytest.raises(engine.KmcError) as e:
            engine.HostPd(p, hs, cfg)
        assert e.value.code == capi.ERR_ARG, kw
    # the bounds themselves
    host = engine.HostPd(p, hs, capi.pd_config(1, 256, 266.0, 400.0, 16384.0))
    assert (host.acc.ncx, host.acc.ncy, host.acc.J, host.acc.F) == (3, 3, 409600, 1 << 24)
    # a box of 2^21 A
    big = params(n_a=3, n_b=2, box_x=2097152.0, box_y=800.0)
    with pytest.raises(engine.KmcError):
        engine.HostPd(big, hs, capi.pd_config(**good))
    # an update off the stride changes nothing; null pointers
    host = engine.HostPd(p, hs, capi.pd_config(**dict(good, every=4)))
    for step in (3, 5, 0):
        with pytest.raises(engine.KmcError):
            host.update(_state(p, step, np.zeros((5, 2))))
    assert host.acc.n_updates == 0 and np.array_equal(host.arrays.U, host.arrays.X0)
    L = engine.load_library()
    v, view, acc = hs.view(), host.arrays.view(), capi.PdOut()
    assert L.kmc_host_pd_begin(C.byref(p), C.byref(v), None, C.byref(view), C.byref(acc)) == capi.ERR_ARG
    assert L.kmc_host_pd_begin(C.byref(p), C.byref(v), C.byref(capi.pd_config(**good)), None, C.byref(acc)) == capi.ERR_ARG
    assert L.kmc_host_pd_update(C.byref(p), C.byref(v), C.byref(view), None, None) == capi.ERR_ARG
    assert L.kmc_host_pd_sample(C.byref(p), C.byref(view), C.byref(host.acc), None, None, None, None) == capi.ERR_ARG
    out = capi.PdOut()  # the tables are optional
    assert L.kmc_host_pd_sample(C.byref(p), C.byref(view), C.byref(host.acc), C.byref(out), None, None,
                                None) == capi.KMC_OK and out.ncx == 10
