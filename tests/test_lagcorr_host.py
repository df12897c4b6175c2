"""Host side of the lag correlator: the sequential counterpart
kmc_host_lag_* (engine.HostLag) against the plain-Python recorder of
tests/_lagcorr.py on sequences of hand-made states, with the values that can be
worked out by hand asserted as such; analysis.lag_curves and the addition of
samples through analysis.reduce_counts.  Every comparison of the two recorders
is exact equality.  No device needed."""
import importlib
import math

import numpy as np
import pytest

from _kmc import PKG, capi, engine, params
from _lagcorr import (RefLag, add_tables, n_rows, pairs_closed_form, row_of, same_arrays, same_sample,
                      sample_tables)

analysis = importlib.import_module(PKG + ".analysis")

BOX = dict(box_x=1000.0, box_y=800.0)   # BX = 1 024 000, BY = 819 200
Q = 1.0 / 1024.0                         # the coordinate quantum, A


def _state(p, step, xy, a_links=None, b_links=None):
    """A host state that holds only what the recorder reads: xy[N, 2] of bead [1][1]; a_links[i] = (nei2, nei4,
    nei3) of receptor i + 1, b_links[i] = (nei2, nei3, nei4) of ligand i + 1."""
    hs = capi.HostState(p.n_a, p.n_b)
    xy = np.asarray(xy, dtype=np.float64)
    hs.ra[0], hs.ra[1] = xy[:p.n_a, 0], xy[:p.n_a, 1]
    hs.rb[0], hs.rb[1] = xy[p.n_a:, 0], xy[p.n_a:, 1]
    for i, l in enumerate(a_links or []):
        hs.a_int[2, i], hs.a_int[3, i], hs.a_int[4, i] = l
    for i, l in enumerate(b_links or []):
        hs.b_int[5, i], hs.b_int[6, i], hs.b_int[7, i] = l
    hs.step = step
    return hs


def _both(p, hs, every, levels, slots, max_jump=0.0, max_disp=0.0, h=(), log=None):
    cfg = capi.lag_config(every, levels, slots, max_jump, max_disp, h)
    return engine.HostLag(p, hs, cfg), RefLag(p, hs, every, levels, slots, max_jump, max_disp, h, log=log)


def _advance(host, ref, hs):
    info = host.update(hs)
    ref.update(hs)
    assert (info.n_updates, info.n_tasks, info.n_events) == (ref.n, ref.last_tasks, ref.last_events)
    assert same_arrays(host.arrays.U, host.arrays.last_event, ref)


def _walk(p, every, n_updates, seed, amp=3.0, step0=0):
    """States of a random walk on the coordinate grid (free of the seam's rounding: multiples of 2^-10 A)."""
    rng = np.random.default_rng(seed)
    n = p.n_a + p.n_b
    box = np.array([p.box_x, p.box_y])
    xy = np.floor(rng.random((n, 2)) * box * 1024.0) * Q
    out = [_state(p, step0, xy)]
    for k in range(1, n_updates + 1):
        xy = np.mod(xy + np.round(rng.normal(0.0, amp, (n, 2)) * 1024.0) * Q, box)
        out.append(_state(p, step0 + k * every, xy))
    return out


def test_schedule_alone():
    # L = 3, P = 4, 40 updates: every row's n_pairs is the closed form; the walk makes every pair term differ
    p = params(n_a=3, n_b=2, **BOX)
    states = _walk(p, 5, 40, seed=1)
    host, ref = _both(p, states[0], 5, 3, 4, h=(1, 3))
    assert n_rows(3, 4) == 8 and host.sample().rows == 8
    for k, hs in enumerate(states[1:], 1):
        _advance(host, ref, hs)
        if k in (1, 3, 4, 7, 8, 16, 40):
            s = host.sample()
            assert same_sample(s, ref)
            assert [int(v) for v in s.n_pairs] == pairs_closed_form(3, 4, k)
    s = host.sample()
    # worked by hand: level 0 row j - 1 holds 41 - j pairs; level 1 (n even, n >= 2 j): j = 3 -> 18, j = 4 -> 17;
    # level 2 (n mod 4 == 0, n >= 4 j): j = 3 -> 8, j = 4 -> 7
    assert [int(v) for v in s.n_pairs] == [40, 39, 38, 37, 18, 17, 8, 7]
    assert [int(v) for v in s.lags] == [1, 2, 3, 4, 6, 8, 12, 16]
    # every pair is clean (no links, steps far below J) and every protein counts in every pair
    assert int(s.n_clean.sum()) == int(s.n_all.sum()) == 5 * sum(int(v) for v in s.n_pairs) and int(s.n_far.sum()) == 0
    # the level above repeats no lag of the level below and leaves none out
    assert (row_of(1, 3, 4), row_of(1, 4, 4), row_of(2, 3, 4)) == (4, 5, 6)


def test_seam_both_directions_both_axes():
    p = params(n_a=2, n_b=2, **BOX)
    # protein 0 crosses +x, 1 crosses -x, 2 crosses +y, 3 crosses -y, each by 1 A per update, then back again
    xy0 = np.array([[999.5, 10.0], [0.25, 20.0], [30.0, 799.5], [40.0, 0.25]])
    move = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    box = np.array([p.box_x, p.box_y])
    host, ref = _both(p, _state(p, 0, xy0), 2, 2, 2, h=(1,))
    xy = xy0
    for k in range(1, 5):
        xy = np.mod(xy + (move if k <= 2 else -move), box)
        _advance(host, ref, _state(p, 2 * k, xy))
        want = np.round(xy0 * 1024.0).astype(np.int64) + (np.round(move * 1024.0).astype(np.int64) * (k if k <= 2 else 4 - k))
        assert np.array_equal(host.arrays.U, want)  # unwrapped: beyond the box and below zero
    assert ref.crossed.all()
    assert host.arrays.U[0, 0] == 1023488 and not host.arrays.last_event.any()
    s = host.sample()
    assert same_sample(s, ref)
    # lag 1 (row 0): four updates, each protein moved 1024 units: q = 2^20 in every pair, all clean
    assert int(s.m2_clean[0].sum()) == 4 * 4 * 2 ** 20 and int(s.m4_clean[0].sum()) == 4 * 4 * 2 ** 40
    # lag 2 (row 1): updates 2, 3, 4 against 0, 1, 2: displacements 2, 0, 2 A
    assert int(s.m2_clean[1].sum()) == 4 * (2 * 2048 ** 2)


def test_link_change_before_at_after_an_origin():
    # receptor 0 takes ligand 3 (N = 3: receptors 0, 1, ligand 2 -> global number 3) at update 3, nothing moves
    p = params(n_a=2, n_b=1, **BOX)
    xy = np.array([[100.0, 100.0], [200.0, 200.0], [300.0, 300.0]])
    free, bound = [(0, 0, 0), (0, 0, 0)], [(3, 2, 0), (0, 0, 0)]
    log = []
    host, ref = _both(p, _state(p, 0, xy, free, [(0, 0, 0)]), 1, 2, 4, log=log)
    for n in range(1, 9):
        a = bound if n >= 3 else free
        b = [(1, 0, 0)] if n >= 3 else [(0, 0, 0)]
        _advance(host, ref, _state(p, n, xy, a, b))
    assert list(host.arrays.last_event) == [3, 0, 3]
    assert same_sample(host.sample(), ref)
    for n, nk, row, i, far, clean in log:
        assert not far
        # only the origins stored before the change (n_k < 3) lose the pair, and only once the change was seen
        assert clean == (not (i in (0, 2) and nk < 3 <= n)), (n, nk, i)
    # the pair of update 3 with the origin of update 3's own slot is filed later as a clean one: (n, n_k) = (4, 3)
    assert (4, 3, 0, 0, False, True) in log and (3, 2, 0, 0, False, False) in log
    s = host.sample()
    # classes follow the current state: receptor 0 counts as class 0 up to update 2 and as class 2 from 3 on
    assert int(s.n_all[0, 0]) == 2 + 8 and int(s.n_all[0, 2]) == 6 and int(s.n_all[0, 3]) == 2 and int(s.n_all[0, 4]) == 6
    assert int(s.n_clean[0, 2]) == 5 and int(s.n_clean[0, 4]) == 5  # lag 1: (3, 2) is the one unclean pair


def test_jump_of_exactly_J_and_one_below():
    p = params(n_a=2, n_b=2, **BOX)
    xy0 = np.array([[100.0, 100.0], [200.0, 200.0], [300.0, 300.0], [400.0, 400.0]])
    host, ref = _both(p, _state(p, 0, xy0), 1, 1, 2, max_jump=10.0)
    assert ref.J == 10240
    d = np.array([[10.0, 0.0], [10.0 - Q, 0.0], [0.0, -10.0], [0.0, -(10.0 - Q)]])  # J, J - 1 in x; -J, -(J - 1) in y
    _advance(host, ref, _state(p, 1, xy0 + d))
    assert list(host.arrays.last_event) == [1, 0, 1, 0]
    _advance(host, ref, _state(p, 2, xy0 + d))
    s = host.sample()
    assert same_sample(s, ref)
    # lag 1: update 1 against origin 0 — the two jumpers are unclean; update 2 against origin 1 — all clean
    assert int(s.n_all[0].sum()) == 8 and int(s.n_clean[0].sum()) == 6
    # lag 2: update 2 against origin 0
    assert int(s.n_all[1].sum()) == 4 and int(s.n_clean[1].sum()) == 2


@pytest.mark.parametrize("max_disp,box", [(50.0, 1000.0), (0.0, 16384.0)])
def test_displacement_of_exactly_F_and_one_below(max_disp, box):
    # four updates of a quarter of F each: protein 0 ends at exactly F from the origin of update 0 in x, protein 1
    # one unit below it in both axes (q just below 2 F^2: the largest sums), protein 2 at -F in y, protein 3 rests.
    # max_jump = half the box keeps the steps from counting as jumps.
    p = params(n_a=2, n_b=2, box_x=box, box_y=box)
    host, ref = _both(p, _state(p, 0, np.zeros((4, 2))), 3, 1, 4, max_jump=0.5 * box, max_disp=max_disp, h=(1, 64))
    F = ref.F
    assert F == (51200 if max_disp else 2 ** 24) and F % 4 == 0
    U = np.zeros((4, 2), dtype=np.int64)
    for k in range(1, 5):
        last = k == 4
        U[0] += (F // 4, 0)
        U[1] += (F // 4 - last, F // 4 - last)
        U[2] += (0, -(F // 4))
        _advance(host, ref, _state(p, 3 * k, np.mod(U * Q, box)))
    assert np.array_equal(host.arrays.U, U) and not host.arrays.last_event.any()
    s = host.sample()
    assert same_sample(s, ref)
    row = 3  # lag 4: the one pair of update 4 with origin 0
    assert int(s.n_pairs[row]) == 1
    assert [int(s.n_far[row, c]) for c in (0, 3)] == [1, 1]      # protein 0 (receptor), protein 2 (ligand)
    assert [int(s.n_all[row, c]) for c in (0, 3)] == [1, 1]      # protein 1, protein 3
    assert int(s.m2_clean[row, 0]) == 2 * (F - 1) ** 2 and int(s.m4_clean[row, 0]) == (2 * (F - 1) ** 2) ** 2
    assert int(s.m2_clean[row, 3]) == 0 and [int(v) for v in s.fs[row, 3]] == [2 ** 31, 2 ** 31]
    assert int(s.n_far.sum()) == 2


@pytest.mark.parametrize("levels,slots,n_updates", [(1, 2, 9), (2, 2, 9), (20, 2, 40), (20, 16, 70), (3, 16, 50)])
def test_shapes_of_the_rings(levels, slots, n_updates):
    p = params(n_a=4, n_b=3, **BOX)
    states = _walk(p, 2, n_updates, seed=levels * 100 + slots)
    host, ref = _both(p, states[0], 2, levels, slots, h=(2,))
    assert host.sample().rows == n_rows(levels, slots) <= capi.LAG_MAX_ROWS
    for hs in states[1:]:
        _advance(host, ref, hs)
    s = host.sample()
    assert same_sample(s, ref)
    assert [int(v) for v in s.n_pairs] == pairs_closed_form(levels, slots, n_updates)
    assert np.array_equal(s.lags, capi.lag_row_lags(levels, slots))


@pytest.mark.parametrize("h", [(), (1, 64, 7, 64)])
def test_multipliers(h):
    p = params(n_a=5, n_b=4, **BOX)
    states = _walk(p, 1, 12, seed=7, amp=40.0)
    host, ref = _both(p, states[0], 1, 2, 4, h=h)
    for hs in states[1:]:
        _advance(host, ref, hs)
    s = host.sample()
    assert same_sample(s, ref)
    assert s.fs.shape == (6, 5, len(h)) and s.nq == len(h)
    if h:
        # a cosine sum below its count, and h = 64 decorrelates where h = 1 has not: the terms are really per multiplier
        n = int(s.n_clean[0, 0])
        assert n > 0 and abs(int(s.fs[0, 0, 0])) <= n * (2 ** 31 + 2)
        assert int(s.fs[0, 0, 1]) == int(s.fs[0, 0, 3]) != int(s.fs[0, 0, 0])


def test_two_recorders_add_through_reduce_counts():
    p = params(n_a=6, n_b=5, **BOX)
    states = _walk(p, 4, 24, seed=11, amp=20.0)
    args = (4, 3, 4, 30.0, 60.0, (1, 5))  # (a small J and F: unclean and far pairs take part in the addition)
    a, ra = _both(p, states[0], *args)
    for hs in states[1:13]:
        _advance(a, ra, hs)
    b, rb = _both(p, states[12], *args)
    for hs in states[13:]:
        _advance(b, rb, hs)
    sa, sb = a.sample(), b.sample()
    assert int(sa.n_far.sum()) > 0 and int(sa.n_clean.sum()) < int(sa.n_all.sum())
    total = sa.from_counts(analysis.reduce_counts(sa.counts()) + analysis.reduce_counts(sb.counts()))
    assert sample_tables(total) == add_tables(ra.tables(), rb.tables())
    # the vector's limbs put negative sums back together too
    neg = sa.from_counts(-sa.counts())
    assert int(neg.m4_clean[0, 0]) == -int(sa.m4_clean[0, 0]) and int(neg.fs[1, 3, 1]) == -int(sa.fs[1, 3, 1])


def test_lag_curves_on_a_hand_written_table():
    out = capi.LagOut()
    out.cfg = capi.lag_config(5, 2, 2, 100.0, 200.0, (1, 3))
    out.BX, out.BY, out.rows = 1024000, 512000, 3
    table = np.zeros((3, capi.LAG_CLASSES), dtype=capi.LAG_CELL_DTYPE)
    c = table[1, 2]
    c["n_all"], c["n_clean"], c["n_far"] = 6, 4, 2
    c["m2_all"]["lo"] = 9 << 20
    c["m2_clean"]["lo"] = 8 << 20                    # <q> = 2 A^2
    c["m4_clean"]["lo"], c["m4_clean"]["hi"] = (48 << 40) & (2 ** 64 - 1), (48 << 40) >> 64  # <q^2> = 12 A^4
    c["fs"][0]["lo"] = 4 << 30                       # mean of the two cosines: 1/2
    c["fs"][1]["lo"], c["fs"][1]["hi"] = 2 ** 64 - (2 << 30), -1   # -(2 << 30): mean -1/4
    s = capi.LagSample(out, table, np.array([7, 6, 3]))
    cur = analysis.lag_curves(s, time_step=10.0)
    assert list(cur["tau"]) == [50.0, 100.0, 200.0]   # lags 1, 2 (level 0) and 4 (level 1, j = 2), 5 steps of 10 ns
    assert cur["msd"][1, 2] == 2.0 and cur["msd_all"][1, 2] == 1.5
    assert cur["alpha2"][1, 2] == 12.0 / (2.0 * 4.0) - 1.0
    assert list(cur["fs"][1, 2]) == [0.5, -0.25]
    assert cur["clean_fraction"][1, 2] == 0.5 and cur["n_clean"][1, 2] == 4.0
    assert np.allclose(cur["q"], [[2 * math.pi / 1000.0, 2 * math.pi / 500.0], [6 * math.pi / 1000.0, 6 * math.pi / 500.0]])
    # zeros where a denominator is zero
    for k in ("msd", "msd_all", "alpha2", "clean_fraction"):
        assert cur[k][0].sum() == 0.0 and cur[k][2, 4] == 0.0
    assert not cur["fs"][0].any()
    # a free two-dimensional Gaussian walk has alpha_2 = 0: q exponential, <q^2> = 2 <q>^2
    table[:] = 0
    table[0, 0]["n_clean"], table[0, 0]["m2_clean"]["lo"], table[0, 0]["m4_clean"]["lo"] = 10, 10 * 3, 10 * 18
    assert analysis.lag_curves(capi.LagSample(out, table, np.array([1, 0, 0])), 1.0)["alpha2"][0, 0] == 0.0


def _begin_rc(p, hs, cfg):
    with pytest.raises(engine.KmcError) as e:
        engine.HostLag(p, hs, cfg)
    return e.value.code


def test_every_argument_error():
    p = params(n_a=2, n_b=1, **BOX)
    hs = _state(p, 0, np.zeros((3, 2)))
    ok = dict(every=1, levels=2, slots=4, max_jump=0.0, max_disp=0.0, h=(1,))
    engine.HostLag(p, hs, capi.lag_config(**ok))
    bad = [dict(slots=3), dict(slots=15), dict(slots=0), dict(slots=18), dict(levels=0), dict(levels=21),
           dict(every=0), dict(every=-3), dict(h=(0,)), dict(h=(1, 65)), dict(h=(-1,)),
           dict(max_jump=float("nan")), dict(max_jump=400.0 + Q), dict(max_jump=float("inf")),
           dict(max_disp=float("nan")), dict(max_disp=16384.0 + Q), dict(max_disp=float("inf"))]
    for kw in bad:
        assert _begin_rc(p, hs, capi.lag_config(**{**ok, **kw})) == -1, kw
    cfg = capi.lag_config(**ok)
    cfg.nq = 5
    assert _begin_rc(p, hs, cfg) == -1
    cfg.nq = -1
    assert _begin_rc(p, hs, cfg) == -1
    # the bounds themselves are legal: half the box, 16384 A, 20 levels, 16 slots, h = 64
    h = engine.HostLag(p, hs, capi.lag_config(7, 20, 16, 400.0, 16384.0, (64, 1, 64, 1)))
    assert (h.acc.J, h.acc.F, h.acc.rows) == (409600, 2 ** 24, 168)
    # a box below the coordinate quantum
    tiny = params(n_a=2, n_b=1, box_x=1.0 / 4096.0, box_y=800.0)
    assert _begin_rc(tiny, hs, capi.lag_config(**ok)) == -1
    # an update off the stride changes nothing
    host, ref = _both(p, hs, 5, 2, 4)
    for step in (0, 4, 6, 10):
        with pytest.raises(engine.KmcError) as e:
            host.update(_state(p, step, np.ones((3, 2))))
        assert e.value.code == -1
    assert host.acc.n_updates == 0 and not host.arrays.U.any() and not host.arrays.n_pairs.any()
    _advance(host, ref, _state(p, 5, np.ones((3, 2))))
    with pytest.raises(engine.KmcError):
        host.update(_state(p, 5, np.ones((3, 2))))
    _advance(host, ref, _state(p, 10, np.ones((3, 2))))
    assert same_sample(host.sample(), ref)
    # null pointers
    L = engine.load_library()
    assert L.kmc_host_lag_begin(None, None, None, None, None) == -1
    assert L.kmc_host_lag_update(None, None, None, None, None) == -1
    assert L.kmc_host_lag_sample(None, None, None, None, None, None) == -1
