"""Host side of the body dynamics: the sequential counterpart
kmc_host_bd_* (engine.HostBd) against the Python reference of tests/_bodydyn.py
on hand-built states and sequences, with the values that can be worked out by
hand asserted as such; analysis.body_msd / body_diffusion / body_rotation /
body_survival and the addition of samples through analysis.reduce_counts.
Every comparison of the two recorders is exact equality.  No device needed."""
import ctypes as C
import importlib

import numpy as np
import pytest

from _bodydyn import (RefBd, blank_state, body_tuples, cis, get_xy, identities, path, put_xy, row_tuples, same_arrays,
                      same_sample, sample_table, set_xy, unbind)
from _kmc import PKG, capi, engine, params

analysis = importlib.import_module(PKG + ".analysis")

BOX = dict(box_x=1000.0, box_y=800.0)   # BX = 1 024 000, BY = 819 200
Q = 1.0 / 1024.0                         # the coordinate quantum, A
ONE = 1 << 30                            # a cosine of 1 in fixed point


def _both(p, hs, every=1, max_size=8, max_jump=0.0, max_disp=0.0):
    host = engine.HostBd(p, hs, capi.bd_config(every, max_size, max_jump, max_disp))
    ref = RefBd(p, hs, every, max_size, max_jump, max_disp)
    a = host.arrays
    assert same_arrays(a.U, a.X0, a.flags, a.label, a.D0, ref) and np.array_equal(a.bits, ref.bits)
    assert (host.acc.J, host.acc.F, host.acc.n_bodies) == (ref.J, ref.F, len(ref.members))
    return host, ref


def _advance(host, ref, hs):
    info = host.update(hs)
    assert (info.n_updates, info.n_jumped, info.n_changed) == (ref.n + 1,) + ref.update(hs)
    a = host.arrays
    assert same_arrays(a.U, a.X0, a.flags, a.label, a.D0, ref) and np.array_equal(a.prev, ref.prev)
    assert np.array_equal(a.links.T, ref.links)


def _same(host, ref, hs):
    s = host.sample(hs)
    t, rows = ref.table(hs)
    assert same_sample(s, ref, t) and s.n_updates == ref.n
    assert body_tuples(host.bodies(hs)) == row_tuples(rows)
    identities(t)
    return s, t, {r["label"]: r for r in rows}


def _moved(hs, step, move=None, xy=None, box=None):
    """A copy of hs at `step` with bead [1][1] of every protein moved by move[N, 2] (or put at xy), wrapped."""
    out = hs.copy()
    out.step = step
    new = get_xy(hs) + move if xy is None else xy
    put_xy(out, np.mod(new, box) if box is not None else new)
    return out


def test_dimer_translated_as_one_and_a_monomer():
    # receptors 0 = 1 cis-bound, 10 A apart along x; receptor 2 alone; the dimer moves (3, -2) A per update
    p = params(n_a=3, n_b=0, **BOX)
    hs = blank_state(p)
    for i, (x, y) in enumerate(((100.0, 100.0), (110.0, 100.0), (500.0, 500.0))):
        set_xy(hs, i, x, y)
    cis(hs, 0, 1)
    host, ref = _both(p, hs)
    s, t, rows = _same(host, ref, hs)
    # the origin: everything pristine, nothing moved, cos phi = 1 for every body with a rotation
    assert t["n_bodies"][0][:3] == [0, 1, 1] == t["n_pristine"][0][:3] == t["n_valid"][0][:3] == t["n_intact"][0][:3]
    assert t["n_rot"][0][2] == 1 and t["c1"][0][2] == t["c2"][0][2] == ONE and t["m2"][0][2] == t["phi2"][0][2] == 0
    assert ref.D0.tolist() == [[0, 0], [10240, 0], [0, 0]]
    move = np.array([[3.0, -2.0], [3.0, -2.0], [0.0, 0.0]])
    for k in (1, 2):
        hs = _moved(hs, k, move)
        _advance(host, ref, hs)
    s, t, rows = _same(host, ref, hs)
    d = rows[1]
    assert (d["su_x"], d["su_y"]) == (2 * 6144, -2 * 4096) and d["S"] == 0 and d["C"] == 10240 ** 2 and d["phi"] == 0.0
    assert t["m2"][0][2] == (2 * 6144) ** 2 + (2 * 4096) ** 2 and t["c1"][0][2] == t["c2"][0][2] == ONE
    assert t["phi2"][0][2] == 0 and t["m2"][0][1] == 0 and t["n_rot"][0][1] == 0 == t["n_rot_skipped"][0][1]
    msd, n_valid = analysis.body_msd(s)
    assert msd[0, 2] == (6.0 ** 2 + 4.0 ** 2) and msd[0, 1] == 0.0 and n_valid[0, 2] == 1 and np.isnan(msd[1, 2])
    rot = analysis.body_rotation(s)
    assert rot["c1"][0, 2] == 1.0 and rot["c2"][0, 2] == 1.0 and rot["phi2"][0, 2] == 0.0 and np.isnan(rot["c1"][0, 1])


@pytest.mark.parametrize("sense", [1, -1])
def test_trimer_rotated_by_a_right_angle_on_the_grid(sense):
    # R0 - L - R1: D0 = (0, 0), (10, 0), (10, 10) A; the relative vectors turn by +-90 degrees about the root
    p = params(n_a=2, n_b=1, **BOX)
    hs = blank_state(p)
    mem = path(hs, iter(range(2)), iter(range(1)), 3)
    assert mem == [0, 2, 1]
    for i, (x, y) in zip(mem, ((100.0, 100.0), (110.0, 100.0), (110.0, 110.0))):
        set_xy(hs, i, x, y)
    host, ref = _both(p, hs)
    assert ref.D0.tolist() == [[0, 0], [10240, 10240], [10240, 0]]
    new = hs.copy()
    new.step = 1
    for i, (x, y) in zip(mem, ((0.0, 0.0), (0.0, 10.0), (-10.0, 10.0))):  # (x, y) -> sense * (-y, x)
        set_xy(new, i, 100.0 + sense * x, 100.0 + sense * y)
    _advance(host, ref, new)
    s, t, rows = _same(host, ref, new)
    d = rows[1]
    assert d["C"] == 0 and d["S"] == sense * 3 * 10240 ** 2 and d["is_"] == 7 and d["status"] == capi.BD_INTACT
    # phi = +-pi/2: cos phi rounds to 0, cos 2 phi to -1, p = round(pi/2 * 2^24) = 26 353 589
    assert t["n_rot"][1][3] == 1 and t["c1"][1][3] == 0 and t["c2"][1][3] == -ONE and t["phi2"][1][3] == 26353589 ** 2
    assert abs(analysis.body_rotation(s)["phi2"][1, 3] - (np.pi / 2) ** 2) < 1e-6
    assert (d["phi"] > 0) == (sense > 0)


def test_c_and_s_both_zero():
    # the second member of a dimer moves onto the root's place: D = 0, no angle
    p = params(n_a=2, n_b=0, **BOX)
    hs = blank_state(p)
    set_xy(hs, 0, 100.0, 100.0)
    set_xy(hs, 1, 110.0, 100.0)
    cis(hs, 0, 1)
    host, ref = _both(p, hs)
    new = _moved(hs, 1, np.array([[0.0, 0.0], [-10.0, 0.0]]))
    _advance(host, ref, new)
    s, t, rows = _same(host, ref, new)
    assert rows[1]["C"] == rows[1]["S"] == 0 and rows[1]["is_"] & capi.BD_IS_ROT
    assert t["n_rot_null"][0][2] == 1 and t["n_rot"][0][2] == 0 and t["c1"][0][2] == 0 and t["n_valid"][0][2] == 1


def test_bodies_across_the_seam_on_each_axis():
    # dimers across the x seam with the root on either side, and across the y seam; then they cross it whole
    p = params(n_a=6, n_b=0, **BOX)
    hs = blank_state(p)
    at = ((999.5, 100.0), (0.5, 100.0), (0.5, 300.0), (999.5, 300.0), (500.0, 799.5), (500.0, 0.5))
    for i, (x, y) in enumerate(at):
        set_xy(hs, i, x, y)
    for a in (0, 2, 4):
        cis(hs, a, a + 1)
    host, ref = _both(p, hs)
    assert ref.shift.tolist() == [[0, 0], [1, 0], [0, 0], [-1, 0], [0, 0], [0, 1]] and not ref.bits.any()
    assert ref.D0.tolist() == [[0, 0], [1024, 0], [0, 0], [-1024, 0], [0, 0], [0, 1024]]
    box = np.array([p.box_x, p.box_y])
    move = np.array([[1.0, 0.0]] * 2 + [[-1.0, 0.0]] * 2 + [[0.0, 1.0]] * 2)
    for k in (1, 2):
        hs = _moved(hs, k, move, box=box)
        _advance(host, ref, hs)
    assert ref.crossed.sum() == 3
    s, t, rows = _same(host, ref, hs)
    assert t["n_rot"][0][2] == 3 and t["c1"][0][2] == 3 * ONE and t["phi2"][0][2] == 0
    assert t["m2"][0][2] == 3 * (2 * 2048) ** 2


def _trimer_and_spare(p):
    """R0 - L - R1 and a free receptor R2, 10 A apart along x."""
    hs = blank_state(p)
    mem = path(hs, iter(range(2)), iter(range(1)), 3)
    for k, i in enumerate(mem + [2]):
        set_xy(hs, i, 100.0 + 10.0 * k, 100.0)
    return hs


def test_a_body_that_loses_a_member_is_broken():
    p = params(n_a=3, n_b=1, **BOX)
    hs = _trimer_and_spare(p)
    host, ref = _both(p, hs)
    new = hs.copy()
    new.step = 1
    unbind(new, 1)
    _advance(host, ref, new)
    assert ref.flags.tolist() == [0, capi.BD_CHANGED, 0, capi.BD_CHANGED]
    s, t, rows = _same(host, ref, new)
    assert rows[1]["status"] == capi.BD_BROKEN and rows[1]["is_"] == 0 and (rows[1]["cur_label"], rows[1]["cur_size"]) == (1, 2)
    assert t["n_broken"][1][3] == 1 and t["n_valid"][1][3] == 0 and t["n_pristine"][0][1] == 1
    surv = analysis.body_survival(s)
    assert surv["broken"][1, 3] == 1.0 and surv["intact"][0, 1] == 1.0 and surv["pristine"][1, 3] == 0.0


def test_a_body_that_gains_a_member_is_grown():
    p = params(n_a=3, n_b=1, **BOX)
    hs = _trimer_and_spare(p)
    host, ref = _both(p, hs)
    new = hs.copy()
    new.step = 1
    cis(new, 1, 2)
    _advance(host, ref, new)
    assert ref.flags.tolist() == [0, capi.BD_CHANGED, capi.BD_CHANGED, 0]
    s, t, rows = _same(host, ref, new)
    assert rows[1]["status"] == capi.BD_GROWN and rows[3]["status"] == capi.BD_GROWN and rows[1]["cur_size"] == 4
    assert t["n_grown"][1][3] == 1 and t["n_grown"][0][1] == 1 and t["n_pristine"][1][3] == 0
    assert analysis.body_survival(s)["grown"][1, 3] == 1.0


@pytest.mark.parametrize("seen", [True, False])
def test_a_body_that_breaks_and_forms_again(seen):
    # seen: the open bond is there at an update, and the body is INTACT but not PRISTINE at the next one; unseen: it
    # opens and closes between two updates, and nothing tells (the caveat of DESIGN.md §21)
    p = params(n_a=3, n_b=1, **BOX)
    hs = _trimer_and_spare(p)
    host, ref = _both(p, hs, every=1 if seen else 2)
    if seen:
        opened = hs.copy()
        opened.step = 1
        unbind(opened, 1)
        _advance(host, ref, opened)
        assert _same(host, ref, opened)[2][1]["status"] == capi.BD_BROKEN
    again = hs.copy()
    again.step = 2
    _advance(host, ref, again)
    s, t, rows = _same(host, ref, again)
    assert rows[1]["status"] == capi.BD_INTACT
    assert bool(rows[1]["is_"] & capi.BD_IS_PRISTINE) == (not seen)
    assert t["n_intact"][1][3] == 1 and t["n_pristine"][1][3] == (0 if seen else 1)


def test_a_jump_of_exactly_j_and_one_unit_below():
    p = params(n_a=4, n_b=0, **BOX)
    hs = blank_state(p)
    for i in range(4):
        set_xy(hs, i, 100.0, 100.0 + 50.0 * i)
    host, ref = _both(p, hs, max_jump=50.0)
    assert ref.J == 51200
    move = np.array([[50.0, 0.0], [50.0 - Q, 0.0], [0.0, -50.0], [0.0, -50.0 + Q]])
    new = _moved(hs, 1, move)
    _advance(host, ref, new)
    assert ref.flags.tolist() == [capi.BD_JUMPED, 0, capi.BD_JUMPED, 0]
    s, t, rows = _same(host, ref, new)
    assert t["n_pristine"][0][1] == 2 and t["n_intact"][0][1] == 4 and t["m2"][0][1] == 2 * 51199 ** 2


def test_a_displacement_of_exactly_f_and_one_unit_below():
    # 64 updates of 256 A: u = 2^24 = F for receptor 0 (and along -y for 2), one quantum less for 1 and 3
    p = params(n_a=4, n_b=0, **BOX)
    hs = blank_state(p)
    for i in range(4):
        set_xy(hs, i, 100.0, 100.0 + 50.0 * i)
    host, ref = _both(p, hs, max_jump=400.0)
    assert ref.F == 1 << 24
    box = np.array([p.box_x, p.box_y])
    move = np.array([[256.0, 0.0], [256.0, 0.0], [0.0, -256.0], [0.0, -256.0]])
    last = move - np.array([[0.0, 0.0], [Q, 0.0], [0.0, 0.0], [0.0, -Q]])
    for k in range(1, 65):
        hs = _moved(hs, k, move if k < 64 else last, box=box)
        _advance(host, ref, hs)
    u = ref.U - ref.X0
    assert u.tolist() == [[1 << 24, 0], [(1 << 24) - 1, 0], [0, -(1 << 24)], [0, -(1 << 24) + 1]] and not ref.flags.any()
    s, t, rows = _same(host, ref, hs)
    assert t["n_pristine"][0][1] == 4 and t["n_valid"][0][1] == 2 and t["m2"][0][1] == 2 * ((1 << 24) - 1) ** 2


def test_a_spanning_body_has_an_msd_and_no_rotation():
    # a ring of six around the box along x: R0 - L0 - R1 = R2 - L1 - R3 = R0
    p = params(n_a=4, n_b=2, **BOX)
    hs = blank_state(p)
    mem = path(hs, iter(range(4)), iter(range(2)), 6)
    cis(hs, mem[-1], mem[0])
    for k, i in enumerate(mem):
        set_xy(hs, i, 10.0 + 166.0 * k, 400.0)
    host, ref = _both(p, hs)
    assert ref.bits.tolist() == [capi.SPAN_X] * 6 and not ref.shift.any()
    new = _moved(hs, 1, np.full((6, 2), 5.0))
    _advance(host, ref, new)
    s, t, rows = _same(host, ref, new)
    assert rows[1]["is_"] == capi.BD_IS_PRISTINE | capi.BD_IS_VALID and rows[1]["C"] == 0
    assert t["n_rot_skipped"][1][6] == 1 and t["n_rot"][1][6] == 0 and t["m2"][1][6] == 2 * (6 * 5120) ** 2
    assert analysis.body_msd(s)[0][1, 6] == 50.0


def test_a_wide_body_at_exactly_2_to_the_24_and_one_below():
    p = params(n_a=4, n_b=0, box_x=40000.0, box_y=40000.0)
    hs = blank_state(p)
    for i, (x, y) in enumerate(((100.0, 100.0), (100.0 + 16384.0, 100.0), (100.0, 900.0), (100.0, 900.0 + 16384.0 - Q))):
        set_xy(hs, i, x, y)
    cis(hs, 0, 1)
    cis(hs, 2, 3)
    host, ref = _both(p, hs)
    assert ref.D0.tolist() == [[0, 0], [1 << 24, 0], [0, 0], [0, (1 << 24) - 1]]
    assert ref.bits.tolist() == [capi.BD_WIDE, capi.BD_WIDE, 0, 0]
    new = _moved(hs, 1, np.full((4, 2), 7.0))
    _advance(host, ref, new)
    s, t, rows = _same(host, ref, new)
    assert rows[1]["is_"] == 3 and rows[3]["is_"] == 7 and rows[3]["C"] == ((1 << 24) - 1) ** 2
    assert t["n_rot_skipped"][0][2] == 1 and t["n_rot"][0][2] == 1 and t["n_valid"][0][2] == 2


def _paths_state(sizes, spacing=1.0, box=4000.0):
    """Paths of the given sizes, each along x on a row of its own (40 A apart), `spacing` between neighbours."""
    n_l = sum((s + 1) // 3 for s in sizes)  # a path is R, L, R, R, L, R, ...
    n_r = sum(sizes) - n_l
    p = params(n_a=n_r, n_b=n_l, box_x=box, box_y=box)
    hs = blank_state(p)
    rec, lig = iter(range(n_r)), iter(range(n_l))
    mems = []
    for row, s in enumerate(sizes):
        mem = path(hs, rec, lig, s)
        for k, i in enumerate(mem):
            set_xy(hs, i, 50.0 + spacing * k, 50.0 + 40.0 * row)
        mems.append(mem)
    assert next(rec, None) is None and next(lig, None) is None
    return p, hs, mems


def test_sizes_max_size_and_one_more_share_the_overflow_row():
    p, hs, mems = _paths_state([4, 5, 3, 1, 2])
    host, ref = _both(p, hs, max_size=4)
    new = _moved(hs, 1, np.full((p.n_a + p.n_b, 2), 3.0))
    _advance(host, ref, new)
    s, t, rows = _same(host, ref, new)
    assert t["n_bodies"][1] == [0, 0, 1, 1, 2] and t["sum_size"][1][4] == 9 and t["n_bodies"][0][:2] == [0, 1]
    assert t["m2"][1][4] == 2 * (4 * 3072) ** 2 + 2 * (5 * 3072) ** 2 and t["n_rot"][1][4] == 2
    msd, _ = analysis.body_msd(s)
    assert np.isnan(msd[1, 4]) and msd[1, 3] == 18.0 and msd[1, 2] == 18.0 and msd[0, 1] == 18.0
    # with the 5 gone the last row holds one size again
    p, hs, mems = _paths_state([4, 4, 3])
    host, ref = _both(p, hs, max_size=4)
    new = _moved(hs, 1, np.full((p.n_a + p.n_b, 2), 3.0))
    _advance(host, ref, new)
    s, t, rows = _same(host, ref, new)
    assert analysis.body_msd(s)[0][1, 4] == 18.0 and analysis.body_rotation(s)["c1"][1, 4] == 1.0


def test_sizes_1023_and_1024_against_the_rotation_cap():
    p, hs, mems = _paths_state([1023, 1024])
    host, ref = _both(p, hs, max_size=capi.BD_MAX_SIZE)
    assert not ref.bits.any() and np.abs(ref.D0).max() == 1023 * 1024
    new = _moved(hs, 1, np.full((p.n_a + p.n_b, 2), -2.0))
    _advance(host, ref, new)
    s, t, rows = _same(host, ref, new)
    small, large = rows[min(mems[0]) + 1], rows[min(mems[1]) + 1]
    assert (small["n_r"] + small["n_l"], small["is_"]) == (1023, 7) and (large["n_r"] + large["n_l"], large["is_"]) == (1024, 3)
    assert small["S"] == 0 and small["C"] == sum((1024 * k) ** 2 for k in range(1023))
    assert t["n_rot"][1][255] == 1 and t["n_rot_skipped"][1][255] == 1 and t["sum_size"][1][255] == 2047


def test_random_walk_of_rigid_and_loose_bodies_and_two_recorders_added():
    # paths of many sizes; every body takes a random rigid step per update, some members a step of their own
    samples = []
    for rec in range(2):
        rng = np.random.default_rng(7 + rec)
        sizes = [1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 9, 12]
        p, hs, mems = _paths_state(sizes, spacing=8.0, box=1000.0)
        hs.step = 10 * rec
        n = p.n_a + p.n_b
        host, ref = _both(p, hs, every=5, max_size=8)
        s, t, rows = _same(host, ref, hs)
        assert all(t["n_pristine"][hl] == t["n_bodies"][hl] == t["n_valid"][hl] for hl in range(2))
        assert all(t["c1"][hl][k] == t["c2"][hl][k] == t["n_rot"][hl][k] * ONE for hl in range(2) for k in range(9))
        assert not any(any(t[name][hl]) for name in ("m2", "phi2") for hl in range(2))
        box = np.array([p.box_x, p.box_y])
        for k in (1, 2):
            move = np.zeros((n, 2))
            for mem in mems:
                move[mem] = np.round(rng.normal(0.0, 20.0, 2) * 1024.0) * Q
            loose = rng.random(n) < 0.15
            move[loose] += np.round(rng.normal(0.0, 3.0, (int(loose.sum()), 2)) * 1024.0) * Q
            hs = _moved(hs, 10 * rec + 5 * k, move, box=box)
            _advance(host, ref, hs)
        s, t, rows = _same(host, ref, hs)
        phis = [r["phi"] for r in rows.values() if r["phi"] is not None]
        assert min(phis) < 0 < max(phis)
        samples.append(s)
    assert samples[0].lag_steps == samples[1].lag_steps == 10
    total = samples[0].from_counts(analysis.reduce_counts(samples[0].counts() + samples[1].counts()))
    a, b, c = (sample_table(x) for x in (samples[0], samples[1], total))
    for name in a:
        assert c[name] == [[x + y for x, y in zip(ra, rb)] for ra, rb in zip(a[name], b[name])], name
    assert np.array_equal(total.from_counts(total.counts()).counts(), total.counts())
    identities(c)


def _hand_sample(max_size=4):
    """A BdSample written by hand: receptor-only bodies of size 1 and 2 and complexes of size 3."""
    table = np.zeros((2, max_size + 1), dtype=capi.BD_CELL_DTYPE)
    out = capi.BdOut()
    out.cfg = capi.bd_config(5, max_size)
    out.origin_step, out.last_step, out.n_bodies = 100, 150, 20
    return out, table


def test_the_analysis_functions_on_a_hand_written_table():
    out, table = _hand_sample()
    # 10 monomers: 8 valid, sum of T = 8 * 4 A^2 * 2^20; 6 dimers: 4 valid, centre MSD 2 A^2 -> m2 = 4 * 2 * 4 * 2^20
    table[0, 1] = (10, 10, 9, 10, 0, 0, 8, 0, 0, 0, 0, 0, (8 * 4 << 20, 0), (0, 0))
    table[0, 2] = (6, 12, 5, 5, 0, 1, 4, 3, 1, 0, 3 * (ONE // 2), -3 * (ONE // 4), (4 * 2 * 4 << 20, 0), (3 << 48, 0))
    table[1, 3] = (4, 12, 1, 2, 1, 1, 0, 0, 0, 0, 0, 0, (0, 0), (0, 0))
    s = capi.BdSample(out, table)
    assert s.lag_steps == 50 and s.total_bodies == 20
    msd, n_valid = analysis.body_msd(s)
    assert msd[0, 1] == 4.0 and msd[0, 2] == 2.0 and np.isnan(msd[1, 3]) and np.isnan(msd[0, 3]) and n_valid[0, 2] == 4
    rot = analysis.body_rotation(s)
    assert rot["c1"][0, 2] == 0.5 and rot["c2"][0, 2] == -0.25 and rot["phi2"][0, 2] == 1.0 and rot["n_rot"][0, 2] == 3
    surv = analysis.body_survival(s)
    assert surv["pristine"][0, 1] == 0.9 and surv["intact"][1, 3] == 0.5 and surv["grown"][1, 3] == 0.25
    assert surv["broken"][1, 3] == 0.25 and np.isnan(surv["intact"][1, 1]) and surv["n_bodies"][0, 2] == 6
    # a second lag at twice the time with twice the MSD: D = MSD / 4t exactly, and D(1) / D(2) = 2 gives gamma = 1
    out2, table2 = _hand_sample()
    out2.last_step = 200
    table2[0, 1] = (10, 10, 9, 10, 0, 0, 8, 0, 0, 0, 0, 0, (8 * 8 << 20, 0), (0, 0))
    table2[0, 2] = (6, 12, 5, 5, 0, 1, 4, 3, 1, 0, 0, 0, (4 * 4 * 4 << 20, 0), (0, 0))
    s2 = capi.BdSample(out2, table2)
    fit = analysis.body_diffusion([(s.lag_steps, s), (s2.lag_steps, s2)], time_step=0.5)
    assert fit["D"][0, 1] == 4.0 / (4 * 25.0) and fit["D"][0, 2] == 2.0 / (4 * 25.0) and fit["n_lags"][0, 2] == 2
    assert abs(fit["gamma"][0] - 1.0) < 1e-12 and np.isnan(fit["gamma"][1]) and np.isnan(fit["D"][1, 3])
    assert np.array_equal(s.from_counts(s.counts()).counts(), s.counts())


def test_bad_arguments():
    p = params(n_a=3, n_b=1, **BOX)
    hs = _trimer_and_spare(p)
    good = dict(every=1, max_size=8, max_jump=0.0, max_disp=0.0)
    for kw in (dict(every=0), dict(max_size=1), dict(max_size=256), dict(max_jump=400.5), dict(max_jump=float("nan")),
               dict(max_disp=16384.5), dict(max_disp=float("nan"))):
        with pytest.raises(engine.KmcError) as e:
            engine.HostBd(p, hs, capi.bd_config(**dict(good, **kw)))
        assert e.value.code == capi.ERR_ARG, kw
    # the bounds themselves
    host = engine.HostBd(p, hs, capi.bd_config(1, 255, 400.0, 16384.0))
    assert (host.acc.J, host.acc.F) == (409600, 1 << 24)
    host = engine.HostBd(p, hs, capi.bd_config(1, 2))
    assert (host.acc.J, host.acc.F, host.acc.cfg.max_jump) == (204800, 1 << 24, 200.0)
    # a box of 2^21 A
    big = params(n_a=3, n_b=1, box_x=2097152.0, box_y=800.0)
    with pytest.raises(engine.KmcError):
        engine.HostBd(big, hs, capi.bd_config(**good))
    # an update off the stride changes nothing; a sample and a list off the last update's step
    host = engine.HostBd(p, hs, capi.bd_config(**dict(good, every=4)))
    for step in (3, 5, 0):
        off = hs.copy()
        off.step = step
        with pytest.raises(engine.KmcError):
            host.update(off)
        if step:
            with pytest.raises(engine.KmcError):
                host.sample(off)
            with pytest.raises(engine.KmcError):
                host.bodies(off)
    assert host.acc.n_updates == 0 and np.array_equal(host.arrays.U, host.arrays.X0)
    # the list: min_size, a capacity too small (the true count comes back), null pointers
    with pytest.raises(engine.KmcError):
        host.bodies(hs, min_size=0)
    with pytest.raises(engine.KmcError) as e:
        host.bodies(hs, cap=1)
    assert e.value.code == capi.ERR_CAPACITY
    assert host.bodies(hs, min_size=2)["label"].tolist() == [1] and len(host.bodies(hs, cap=2)) == 2
    L = engine.load_library()
    v, view, acc, cfg = hs.view(), host.arrays.view(), capi.BdOut(), capi.bd_config(**good)
    assert L.kmc_host_bd_begin(C.byref(p), C.byref(v), None, C.byref(view), C.byref(acc)) == capi.ERR_ARG
    assert L.kmc_host_bd_begin(C.byref(p), C.byref(v), C.byref(cfg), None, C.byref(acc)) == capi.ERR_ARG
    assert L.kmc_host_bd_begin(C.byref(p), C.byref(v), C.byref(cfg), C.byref(view), None) == capi.ERR_ARG
    broken_view = host.arrays.view()
    broken_view.D0 = None
    assert L.kmc_host_bd_begin(C.byref(p), C.byref(v), C.byref(cfg), C.byref(broken_view), C.byref(acc)) == capi.ERR_ARG
    assert L.kmc_host_bd_update(C.byref(p), C.byref(v), C.byref(view), None, None) == capi.ERR_ARG
    assert L.kmc_host_bd_sample(C.byref(p), C.byref(v), C.byref(view), C.byref(host.acc), None, None) == capi.ERR_ARG
    assert L.kmc_host_bd_bodies(C.byref(p), C.byref(v), C.byref(view), C.byref(host.acc), 1, 4, None, None) == capi.ERR_ARG
    # a link that leaves the state
    bad = hs.copy()
    bad.a_int[4, 2] = 77
    with pytest.raises(engine.KmcError) as e:
        engine.HostBd(p, bad, capi.bd_config(**good))
    assert e.value.code == capi.ERR_STATE
