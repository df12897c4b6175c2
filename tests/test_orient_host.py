"""Host side of the orientation layer: the sequential
counterparts kmc_host_rot_* (engine.HostRot) and kmc_host_ligand_pose against
the plain-Python reference of tests/_orient.py on sequences of hand-made states,
with the values that can be worked out by hand asserted as such;
analysis.rot_curves, analysis.pose_profile and the addition of samples through
analysis.reduce_counts.  Every comparison of the two recorders is exact
equality.  No device needed."""
import importlib
import math

import numpy as np
import pytest

from _kmc import PKG, capi, engine, params
from _lagcorr import pairs_closed_form
from _orient import (BAD, RefRot, add_tables, n_rows, pose, same_arrays, same_info, same_pose, same_sample,
                     sample_tables)

analysis = importlib.import_module(PKG + ".analysis")

Q = 1.0 / 1024.0   # the coordinate quantum, A
ARM = 35473        # quanta: 2 * 30 / sqrt 3 A, the longest vector a valid state holds
E = np.eye(3, dtype=np.int64)


def _state(p, step, H, N, A, Cv=None, pos_a=None, pos_b=None, a_links=None, b_links=None):
    """A host state that holds only what the layer reads, from integer vectors in quanta: receptor i has bead [3][1]
    at pos_a[i] and [3][2] at pos_a[i] + H[i]; ligand b has [1][1] at pos_b[b] and [1][2], [2][1], [3][1] at pos_b[b] +
    N[b], A[b], Cv[b] (Cv defaults to N x A / 2^15: a right-handed body).  Links as test_lagcorr_host's."""
    hs = capi.HostState(p.n_a, p.n_b)
    H, N, A = (np.asarray(x, dtype=np.int64).reshape(-1, 3) for x in (H, N, A))
    Cv = np.cross(N, A) // 32768 if Cv is None else np.asarray(Cv, dtype=np.int64).reshape(-1, 3)
    pos_a = np.zeros((p.n_a, 3), dtype=np.int64) + 5 if pos_a is None else np.asarray(pos_a, dtype=np.int64)
    pos_b = np.zeros((p.n_b, 3), dtype=np.int64) + 51200 if pos_b is None else np.asarray(pos_b, dtype=np.int64)

    def put(arr, per_row, j, k, xyz):
        r = ((j - 1) * per_row + (k - 1)) * 3
        for c in range(3):
            arr[r + c] = xyz[:, c] * Q

    put(hs.ra, 4, 3, 1, pos_a)
    put(hs.ra, 4, 3, 2, pos_a + H)
    put(hs.rb, 2, 1, 1, pos_b)
    put(hs.rb, 2, 1, 2, pos_b + N)
    put(hs.rb, 2, 2, 1, pos_b + A)
    put(hs.rb, 2, 3, 1, pos_b + Cv)
    for i, l in enumerate(a_links or []):
        hs.a_int[2, i], hs.a_int[3, i], hs.a_int[4, i] = l
    for i, l in enumerate(b_links or []):
        hs.b_int[5, i], hs.b_int[6, i], hs.b_int[7, i] = l
    hs.step = step
    return hs


def _both(p, hs, every, levels, slots, log=None):
    return engine.HostRot(p, hs, capi.rot_config(every, levels, slots)), RefRot(p, hs, every, levels, slots, log=log)


def _advance(host, ref, hs):
    info = host.update(hs)
    ref.update(hs)
    assert same_info(info, ref)
    assert same_arrays(host.arrays.vec, host.arrays.last_event, host.arrays.chi, ref)
    return info


def _tumble(p, every, n_updates, seed, step0=0):
    """States of bodies that turn at random: headings of 20 A in the plane, ligand frames of 30 A and the arm's
    length turned by random rotations, all rounded to the quantum."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_updates + 1):
        phi = rng.uniform(0, 2 * np.pi, p.n_a)
        H = np.round(np.stack([np.cos(phi), np.sin(phi), 0 * phi], axis=1) * 20480).astype(np.int64)
        R = np.linalg.qr(rng.normal(size=(p.n_b, 3, 3)))[0]
        R[:, :, 2] *= np.sign(np.linalg.det(R))[:, None]  # proper rotations: the handedness stays +1
        N = np.round(R[:, :, 0] * 30720).astype(np.int64)
        A = np.round(R[:, :, 1] * ARM).astype(np.int64)
        Cv = np.round(R[:, :, 2] * 30720).astype(np.int64)
        out.append(_state(p, step0 + k * every, H, N, A, Cv))
    return out


def test_schedule_alone():
    # L = 3, P = 4, 40 updates: every row's n_pairs is the closed form; the tumbling makes every pair term differ
    p = params(n_a=3, n_b=2)
    states = _tumble(p, 5, 40, seed=1)
    host, ref = _both(p, states[0], 5, 3, 4)
    assert n_rows(3, 4) == 8 and host.sample().rows == 8
    for k, hs in enumerate(states[1:], 1):
        _advance(host, ref, hs)
        if k in (1, 3, 4, 7, 8, 16, 40):
            s = host.sample()
            assert same_sample(s, ref)
            assert [int(v) for v in s.n_pairs] == pairs_closed_form(3, 4, k)
    s = host.sample()
    assert [int(v) for v in s.n_pairs] == [40, 39, 38, 37, 18, 17, 8, 7]
    assert [int(v) for v in s.lags] == [1, 2, 3, 4, 6, 8, 12, 16]
    # no links, proper rotations only: every pair is clean; a receptor counts once and a ligand twice in every pair
    assert ref.flips_total == 0 and not host.arrays.last_event.any()
    total = sum(int(v) for v in s.n_pairs)
    assert int(s.n_clean.sum()) == int(s.n_all.sum()) == (3 + 2 * 2) * total
    assert int(s.n_all[:, :3, 1].sum()) == 0 and int(s.n_all[:, 3, 1].sum()) == 2 * total
    assert int(s.s1_clean[0, 0, 0]) != 0 and int(s.s1_clean[0, 3, 1]) != int(s.s1_clean[0, 3, 0])


def test_link_change_before_at_after_an_origin():
    # receptor 0 takes ligand 3 (N = 3: receptors 0, 1, ligand 2 -> global number 3) at update 3, nothing turns
    p = params(n_a=2, n_b=1)
    H, N, A = [[20480, 0, 0], [0, 20480, 0]], [[0, 0, 30720]], [[ARM, 0, 0]]
    free, bound = [(0, 0, 0), (0, 0, 0)], [(3, 2, 0), (0, 0, 0)]
    log = []
    host, ref = _both(p, _state(p, 0, H, N, A, a_links=free, b_links=[(0, 0, 0)]), 1, 2, 4, log=log)
    for n in range(1, 9):
        a = bound if n >= 3 else free
        b = [(1, 0, 0)] if n >= 3 else [(0, 0, 0)]
        info = _advance(host, ref, _state(p, n, H, N, A, a_links=a, b_links=b))
        assert (info.n_events, info.n_flips) == ((2, 0) if n == 3 else (0, 0))
    assert list(host.arrays.last_event) == [3, 0, 3]
    assert same_sample(host.sample(), ref)
    for n, nk, row, i, v, clean in log:
        # only the origins stored before the change (n_k < 3) lose the pair, and only once the change was seen
        assert clean == (not (i in (0, 2) and nk < 3 <= n)), (n, nk, i)
    assert (4, 3, 0, 0, 0, True) in log and (3, 2, 0, 0, 0, False) in log and (3, 2, 0, 2, 1, False) in log
    s = host.sample()
    # classes follow the current state: receptor 0 counts as class 0 up to update 2 and as class 2 from 3 on
    assert int(s.n_all[0, 0, 0]) == 2 + 8 and int(s.n_all[0, 2, 0]) == 6
    assert [int(s.n_all[0, 3, v]) for v in (0, 1)] == [2, 2] and [int(s.n_all[0, 4, v]) for v in (0, 1)] == [6, 6]
    assert int(s.n_clean[0, 2, 0]) == 5 and int(s.n_clean[0, 4, 1]) == 5  # lag 1: (3, 2) is the one unclean pair
    # nothing turned: d = |u|^2 in every pair
    assert int(s.s1_all[0, 0, 0]) == 10 * 20480 ** 2 and int(s.s2_clean[0, 4, 1]) == 5 * ARM ** 4


def test_a_ligand_reflected_between_two_updates():
    # ligand 1 is mirrored at z = 0 between updates 2 and 3 (z -> -z of all its beads); ligand 0 and the receptor rest
    p = params(n_a=1, n_b=2)
    H = [[12288, 16384, 0]]
    N = np.array([[1000, 2000, 30000], [3000, -4000, 25000]])
    A = np.array([[30000, 1000, -1100], [20000, 25000, 1600]])
    Cv = np.array([[-2000, 30000, 900], [-25000, 20000, 6200]])
    pos_b = np.array([[0, 0, 40960], [7, 9, 20480]])
    mirror = np.array([1, 1, -1])
    host, ref = _both(p, _state(p, 0, H, N, A, Cv, pos_b=pos_b), 1, 1, 4)
    chi0 = list(host.arrays.chi)
    assert chi0[0] == 0 and abs(chi0[1]) == 1 and abs(chi0[2]) == 1
    flips = []
    for n in range(1, 7):
        m = n >= 3
        N2, A2, C2, pb = N.copy(), A.copy(), Cv.copy(), pos_b.copy()
        if m:
            N2[1], A2[1], C2[1], pb[1] = N[1] * mirror, A[1] * mirror, Cv[1] * mirror, pos_b[1] * mirror
        flips.append(int(_advance(host, ref, _state(p, n, H, N2, A2, C2, pos_b=pb)).n_flips))
    assert flips == [0, 0, 1, 0, 0, 0] and ref.flips_total == 1
    assert list(host.arrays.chi) == [0, chi0[1], -chi0[2]] and list(host.arrays.last_event) == [0, 0, 3]
    s = host.sample()
    assert same_sample(s, ref)
    # the axis: u . u' with z mirrored = x^2 + y^2 - z^2 for a pair that spans the reflection, |u|^2 otherwise
    n0, n1 = [int(v) for v in (N * N).sum(axis=1)]
    span = 3000 ** 2 + 4000 ** 2 - 25000 ** 2
    # lag 1 (row 0): six pairs a ligand; (3, 2) spans, and is in s1_all and not in s1_clean; (4, 3) on are clean again
    assert int(s.n_all[0, 3, 0]) == 12 and int(s.n_clean[0, 3, 0]) == 11
    assert int(s.s1_all[0, 3, 0]) == 6 * n0 + 5 * n1 + span and int(s.s1_clean[0, 3, 0]) == 6 * n0 + 5 * n1
    # lag 3 (row 2): updates 3..6 against origins 0..3; (3, 0), (4, 1), (5, 2) span, (6, 3) is clean
    assert int(s.n_all[2, 3, 0]) == 8 and int(s.n_clean[2, 3, 0]) == 5
    assert int(s.s1_all[2, 3, 0]) - int(s.s1_clean[2, 3, 0]) == 3 * span
    assert int(s.s2_clean[2, 3, 0]) == 4 * n0 ** 2 + n1 ** 2


def test_component_of_two_to_the_16_is_bad_and_one_below_is_not():
    p = params(n_a=2, n_b=2)
    H = [[65536, 0, 0], [65535, -65535, 0]]
    N = [[0, 0, 65535], [0, 0, 30720]]
    A = [[-65535, 1, 0], [0, -65536, 0]]
    Cv = [[0, 65535, 0], [30720, 0, 0]]
    hs = _state(p, 0, H, N, A, Cv)
    host, ref = _both(p, hs, 1, 1, 2)
    assert [int(w) for w in host.arrays.vec] == [BAD, (65535 & 0x1FFFFF) | ((-65535 & 0x1FFFFF) << 21),
                                                  65535 << 42, BAD, (-65535 & 0x1FFFFF) | (1 << 21), BAD]
    # ligand 0: a x c = (0, 0, -65535^2), n . (a x c) = -65535^3; the bad ligand's handedness is 0
    assert list(host.arrays.chi) == [0, 0, -1, 0]
    for n in (1, 2):
        hs = _state(p, n, H, N, A, Cv)
        info = _advance(host, ref, hs)
        assert (info.n_bad, info.n_events, info.n_flips) == (2, 0, 0)
    s = host.sample()
    assert same_sample(s, ref)
    # receptor 0 and ligand 1 count in n_bad only: one receptor and one ligand file pairs
    assert [int(s.n_all[0, c].sum()) for c in range(5)] == [2, 0, 0, 4, 0] and int(s.n_pairs[0]) == 2
    assert int(s.s1_all[0, 0, 0]) == 2 * 2 * 65535 ** 2 and int(s.s2_clean[0, 3, 0]) == 2 * 65535 ** 4
    assert int(s.s2_clean[0, 0, 0]) == 2 * (2 * 65535 ** 2) ** 2  # d^2 = 2^66 - ...: beyond 64 bits
    # a protein that turns bad later files nothing against its good origins, and later not against its bad one
    host, ref = _both(p, _state(p, 0, [[20480, 0, 0]] * 2, N, [[ARM, 0, 0]] * 2, Cv), 1, 1, 2)
    for n, h0 in ((1, 65536), (2, 20480), (3, 20480)):
        info = _advance(host, ref, _state(p, n, [[h0, 0, 0], [20480, 0, 0]], N, [[ARM, 0, 0]] * 2, Cv))
        assert info.n_bad == (n == 1)
    s = host.sample()
    assert same_sample(s, ref)
    # receptor 0: lag 1 files (3, 2) alone, lag 2 files none ((2, 0) is good-good: it does) -> rows 0 and 1
    assert int(s.n_all[0, 0, 0]) == 3 + 1 and int(s.n_all[1, 0, 0]) == 2 + 1


def test_the_largest_sums():
    # every ligand vector at the arm's bound, d = +-|u|^2: 20481 (1, 1, 1) has |u|^2 = 1 258 414 083 >= 35473^2
    p = params(n_a=64, n_b=64)
    u = np.array([20480, 20480, 0]), np.array([20481, 20481, 20481])
    assert int((u[1] * u[1]).sum()) >= ARM ** 2
    Cv = [[20480, -20480, 0]] * 64

    def st(n):
        sg = -1 if n % 2 else 1  # a turn by pi every update: N and A change sign, C does not — the handedness stays
        return _state(p, n, [u[0] * sg] * 64, [u[1] * sg] * 64, [u[1][::-1] * sg] * 64, Cv)

    host, ref = _both(p, st(0), 1, 2, 2)
    for n in range(1, 9):
        assert _advance(host, ref, st(n)).n_flips == 0
    s = host.sample()
    assert same_sample(s, ref)
    a2, b2 = int((u[0] * u[0]).sum()), int((u[1] * u[1]).sum())
    # lag 1: 8 pairs of opposite vectors; lag 2: 7 pairs of equal ones
    assert int(s.s1_clean[0, 0, 0]) == -8 * 64 * a2 and int(s.s1_clean[1, 0, 0]) == 7 * 64 * a2
    assert int(s.s1_clean[0, 3, 1]) == -8 * 64 * b2 and int(s.s2_clean[0, 3, 1]) == 8 * 64 * b2 ** 2 > 2 ** 64
    assert int(s.s2_clean[1, 3, 0]) == 7 * 64 * b2 ** 2


def test_two_recorders_add_through_reduce_counts():
    p = params(n_a=6, n_b=5)
    states = _tumble(p, 4, 24, seed=11)
    # link changes in both halves: unclean pairs take part in the addition
    for k in (5, 6, 7, 17, 18):
        states[k].a_int[2, 0], states[k].b_int[5, 1] = 8, 1
    a, ra = _both(p, states[0], 4, 3, 4)
    for hs in states[1:13]:
        _advance(a, ra, hs)
    b, rb = _both(p, states[12], 4, 3, 4)
    for hs in states[13:]:
        _advance(b, rb, hs)
    sa, sb = a.sample(), b.sample()
    assert int(sa.n_clean.sum()) < int(sa.n_all.sum()) and int(sb.n_clean.sum()) < int(sb.n_all.sum())
    total = sa.from_counts(analysis.reduce_counts(sa.counts()) + analysis.reduce_counts(sb.counts()))
    assert sample_tables(total) == add_tables(ra.tables(), rb.tables())
    # the vector's limbs put negative sums back together too
    neg = sa.from_counts(-sa.counts())
    assert int(neg.s1_all[0, 0, 0]) == -int(sa.s1_all[0, 0, 0]) != 0 and int(neg.s2_clean[1, 3, 1]) == -int(sa.s2_clean[1, 3, 1])


def test_rot_curves_on_a_hand_written_table():
    p = params(n_a=1, n_b=1, time_step=10.0)   # R_A = 20, R_B = 30
    out = capi.RotOut()
    out.cfg = capi.rot_config(5, 2, 2)
    out.rows = 3
    table = np.zeros((3, capi.LAG_CLASSES, capi.ROT_VECS), dtype=capi.ROT_CELL_DTYPE)
    a2, b2 = 20480 ** 2, 30720 ** 2
    c = table[1, 1, 0]                         # headings: <cos> = 1/2, <cos^2> = 5/8 -> <cos 2 phi> = 1/4
    c["n_all"], c["n_clean"] = 8, 4
    c["s1_all"]["lo"] = 2 * a2
    c["s1_clean"]["lo"] = 2 * a2
    v = 4 * a2 * a2 * 5 // 8
    c["s2_clean"]["lo"], c["s2_clean"]["hi"] = v & (2 ** 64 - 1), v >> 64
    c = table[2, 4, 1]                         # arms (|u|^2 = 4 R_B^2 / 3): <cos> = -1/4, <cos^2> = 1/2 -> P_2 = 1/4
    arm2 = 4 * b2 // 3
    c["n_all"], c["n_clean"] = 2, 2
    c["s1_clean"]["lo"], c["s1_clean"]["hi"] = 2 ** 64 - arm2 // 2, -1
    v = arm2 * arm2
    c["s2_clean"]["lo"], c["s2_clean"]["hi"] = v & (2 ** 64 - 1), v >> 64
    s = capi.RotSample(out, table, np.array([7, 6, 3]))
    assert int(s.s1_clean[2, 4, 1]) == -(arm2 // 2)
    cur = analysis.rot_curves(s, p)
    assert list(cur["tau"]) == [50.0, 100.0, 200.0]
    assert cur["c1"][1, 1, 0] == 0.5 and cur["c2"][1, 1, 0] == 0.25 and cur["c1_all"][1, 1, 0] == 0.25
    assert cur["clean_fraction"][1, 1, 0] == 0.5 and cur["n_clean"][1, 1, 0] == 4.0
    assert math.isclose(cur["c1"][2, 4, 1], -0.25, rel_tol=1e-9) and math.isclose(cur["c2"][2, 4, 1], 0.25, rel_tol=1e-9)
    # zeros where a denominator is zero, and in v = 1 of the receptor classes
    for k in ("c1", "c2", "c1_all", "clean_fraction"):
        assert cur[k][0].sum() == 0.0 and cur[k][2, 3, 0] == 0.0 and not cur[k][:, :3, 1].any()
    assert np.array_equal(analysis.rot_lengths(p), [[a2, 0]] * 3 + [[b2, 4 * b2 / 3]] * 2)


def _rc(f, *a):
    with pytest.raises(engine.KmcError) as e:
        f(*a)
    return e.value.code


def test_every_argument_error():
    p = params(n_a=2, n_b=1)
    H, N, A = [[20480, 0, 0]] * 2, [[0, 0, 30720]], [[ARM, 0, 0]]
    hs = _state(p, 0, H, N, A)
    engine.HostRot(p, hs, capi.rot_config(1, 2, 4))
    for cfg in ((1, 2, 3), (1, 2, 15), (1, 2, 0), (1, 2, 18), (1, 0, 4), (1, 21, 4), (0, 2, 4), (-3, 2, 4)):
        assert _rc(engine.HostRot, p, hs, capi.rot_config(*cfg)) == -1, cfg
    assert engine.HostRot(p, hs, capi.rot_config(7, 20, 16)).acc.rows == 168  # the bounds themselves are legal
    # an update off the stride changes nothing
    host, ref = _both(p, hs, 5, 2, 4)
    before = host.arrays.vec.copy()
    for step in (0, 4, 6, 10):
        assert _rc(host.update, _state(p, step, [[0, 20480, 0]] * 2, N, A)) == -1
    assert host.acc.n_updates == 0 and np.array_equal(host.arrays.vec, before) and not host.arrays.n_pairs.any()
    _advance(host, ref, _state(p, 5, [[0, 20480, 0]] * 2, N, A))
    assert _rc(host.update, _state(p, 5, H, N, A)) == -1
    _advance(host, ref, _state(p, 10, H, N, A))
    assert same_sample(host.sample(), ref)
    # null pointers
    L = engine.load_library()
    assert L.kmc_host_rot_begin(None, None, None, None, None) == -1
    assert L.kmc_host_rot_update(None, None, None, None, None) == -1
    assert L.kmc_host_rot_sample(None, None, None, None, None, None) == -1
    assert L.kmc_host_ligand_pose(None, None, 1, 1, None, None) == -1
    # the pose census' bins
    for nz, nc in ((0, 4), (4, 0), (65, 4), (4, 65), (-1, -1)):
        assert _rc(engine.host_ligand_pose, p, hs, nz, nc) == -1, (nz, nc)
    assert _rc(engine.host_ligand_pose, params(n_a=2, n_b=1, box_z=1.0 / 4096.0), hs, 4, 4) == -1
    v = hs.view()
    out = capi.PoseOut()
    assert L.kmc_host_ligand_pose(p, v, 4, 4, None, out) == 0 and int(out.chi_pos[0]) + int(out.chi_neg[0]) == 1


def test_pose_bins_at_their_edges():
    p = params(n_a=1, n_b=9, box_z=250.0)   # BZ = 256000, Lq = 30720
    BZ, Lq = 256000, 30720
    z = [0, BZ, -40, BZ + 40, BZ - 1, 1, BZ // 2, BZ // 2 - 1, 100]
    nzq = [Lq, -Lq, 0, Lq, -Lq, 0, Lq - 1, -Lq + 1, 1]
    N = [[0, 0, v] if abs(v) == Lq else [3, 4, v] for v in nzq]
    A = [[ARM, 0, 0]] * 9
    Cv = [[0, 1000, 0]] * 8 + [[0, -1000, 0]]
    pos_b = [[10 * b, 0, z[b]] for b in range(9)]
    blinks = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 0, 1), (1, 1, 1), (0, 0, 0), (99, 0, 0), (0, 0, 1), (1, 1, 0)]
    hs = _state(p, 0, [[20480, 0, 0]], N, A, Cv, pos_b=pos_b, b_links=blinks)
    for nz, nc in ((1, 1), (64, 64), (4, 3), (5, 64)):
        got = engine.host_ligand_pose(p, hs, nz, nc)
        assert same_pose(got, p, hs, nz, nc)
        assert int(got[0].sum()) == 9 and int(got[1].n_bad) == 0
    hist, out = engine.host_ligand_pose(p, hs, 4, 4)
    k = [0, 1, 1, 2, 3, 0, 0, 1, 2]  # occupied sites: a link out of range (99) is none
    assert [int(v) for v in hist.sum(axis=(1, 2))] == [k.count(c) for c in range(4)]
    # z = 0 and slightly below: bin 0; z = box_z exactly and above: the last bin; box_z / 2: bin nz / 2, one below it: the bin below
    assert hist[0, 0, 3] == 1 and hist[1, 3, 0] == 1 and hist[1, 0, 1] == 1 and hist[2, 3, 3] == 1 and hist[3, 3, 0] == 1
    assert hist[0, 2, 3] == 1 and hist[1, 1, 0] == 1 and hist[2, 0, 2] == 1 and hist[0, 0, 1] == 1
    # N_z = +Lq (a laid-down ligand) lies in the top bin for every nc, -Lq in bin 0, 0 in the middle
    for nc in (1, 2, 3, 64):
        h, _ = engine.host_ligand_pose(p, hs, 1, nc)
        assert h[0, 0, nc - 1] >= 1 and h[1, 0, 0] >= 1 and h[2, 0, nc - 1] >= 1 and h[3, 0, 0] == 1
        assert h[1, 0, (Lq * nc) // (2 * Lq + 1)] >= 1
    # the handedness: a x c = (0, 0, 1000 ARM), so chi = sign(N_z), but for ligand 8 with the mirrored third vector;
    # N_z = 0 (ligands 2 and 5) is a flat body: chi = 0, in neither count
    assert [int(x) for x in out.chi_pos] == [2, 0, 1, 0] and [int(x) for x in out.chi_neg] == [0, 2, 1, 1]
    # a bad ligand counts in n_bad alone
    N[2] = [0, 65536, 0]
    hist, out = engine.host_ligand_pose(p, _state(p, 0, [[20480, 0, 0]], N, A, Cv, pos_b=pos_b, b_links=blinks), 4, 4)
    assert int(out.n_bad) == 1 and int(hist.sum()) == 8 and sum(out.chi_pos) + sum(out.chi_neg) == 7
    prof = analysis.pose_profile(hist, p)
    assert np.allclose(prof["z"], [31.25, 93.75, 156.25, 218.75]) and np.allclose(prof["cos"], -prof["cos"][::-1])
    assert np.allclose(prof["pdf"].sum(axis=(1, 2)), 1.0) and list(prof["n"]) == [3.0, 2.0, 2.0, 1.0]
    assert np.allclose(prof["pdf_z"].sum(axis=1), 1.0) and np.allclose(prof["pdf_cos"].sum(axis=1), 1.0)
    assert pose(p, hs, 4, 4)[3] == 0
