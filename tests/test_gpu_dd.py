"""The slab windows' device checks, one entry point at a time (kmc_dd_* of
include/kmc.h: k_dd_pack / unpack / import / export / jumpers / jumpers_rep /
drift, the cross-bond list of the matching kernels, kmc_dd_finish,
kmc_dd_cut_count).

test_gpu_slabs.py compares whole decomposed trajectories: it notices a wrong
*state*, not a *check* that never fires.  Here the G = 3 windows of one evolved
state are set on engine handles and on keyed oracle windows (oracle_dd_*, the
sequential restatement: the reference of every comparison, by equality), and
every report, list, flag and row the protocol produces is compared — in
lockstep over real steps, and on crafted rows for the cases real steps rarely
make (a cut link in the band, the sign of zero, a status that alone differs).
"""
import ctypes as C

import numpy as np
import pytest

from _dd import (ROW, Family, OracleWindow, bond_set, capi, evolved, jumper_set, report_fields, same_export)
from _kmc import engine

pytestmark = pytest.mark.gpu

G = 3
T_EVOLVE = 400   # whole-box oracle steps before the windows are cut (≈ 200 bonds)
STEPS = 40       # lockstep steps: a cross-slab bond forms at the 4th, a halo link differs at the 32nd
S_LIST = 30.0    # the lockstep's jumper threshold: a few listed per step, never more than KMC_DD_JCAP
COUNTS = ("bad", "differed", "links", "n_xb", "xcol", "xbond")  # the report without the jumpers


def window_handle(q):
    return engine.Simulation(q, device=0)


def raw_jumpers(sim, S, cap):
    """kmc_dd_jumpers itself with room for `cap`: (*n, ids[cap], xs[cap]); one
    more element than cap is passed and must come back untouched."""
    ids = np.full(cap + 1, -7, dtype=np.int32)
    xs = np.full(cap + 1, -7.0)
    n = C.c_int32(-1)
    rc = engine.load_library().kmc_dd_jumpers(sim._h, S, cap, ids.ctypes.data, xs.ctypes.data, C.byref(n))
    assert rc == 0 and ids[cap] == -7 and xs[cap] == -7.0
    return int(n.value), ids[:cap], xs[:cap]


def families():
    p, hs = evolved(T_EVOLVE)
    return p, Family(p, hs.copy(), G, window_handle), Family(p, hs.copy(), G, OracleWindow)


def ints_of(rows):
    return np.ascontiguousarray(rows[:, 384:]).view(np.int32)


def set_int(rows, i, f, v):
    rows[i, 384 + 4 * f:388 + 4 * f] = np.array([v], dtype=np.int32).view(np.uint8)


def set_bead(rows, i, e, v):
    rows[i, 8 * e:8 * e + 8] = np.array([v], dtype=np.float64).view(np.uint8)


def bead_of(rows, i, e):
    return float(rows[i, 8 * e:8 * e + 8].copy().view(np.float64)[0])


def check_preconditions(p, fam):
    """A regenerated state must not empty the tests: every window holds fewer
    proteins than the box and receives a receptor–ligand and a cis bond."""
    for k, r in enumerate(fam.ranks):
        assert r.win.gids.size < p.n_a + p.n_b
        ids = fam.recv_ids(k)
        assert ids.size == r.n_recv > capi.DD_JCAP
        _, ints = r.eng.dd_export(ids)
        rec = ids < r.win.n_a
        assert (rec & (ints[:, 2] > 0)).any() and (rec & (ints[:, 4] > 0)).any()


def compare_windows(E, Or, where):
    """Everything a window can be asked after a finish, engine against oracle."""
    for k in range(G):
        e, o = E.ranks[k], Or.ranks[k]
        every = np.arange(e.win.gids.size, dtype=np.int32)
        band = np.flatnonzero(e.win.band).astype(np.int32)
        assert e.eng.dd_cut_count(every) == o.eng.dd_cut_count(every), (where, k)
        assert e.eng.dd_cut_count(band) == o.eng.dd_cut_count(band), (where, k)
        assert e.eng.dd_drift() == o.eng.dd_drift(), (where, k)
        assert e.eng.dd_counters() == o.eng.dd_counters(), (where, k)
        assert same_export(E.export_all(k), Or.export_all(k)), (where, k)


@pytest.mark.parametrize("resort", [None, "3"])
def test_lockstep_protocol(monkeypatch, resort):
    # KMC_RESORT=3: the slots are re-sorted every third step, so slot_of /
    # id_of are not the identity in any of the window kernels
    if resort is None:
        monkeypatch.delenv("KMC_RESORT", raising=False)
    else:
        monkeypatch.setenv("KMC_RESORT", resort)
    p, E, Or = families()
    try:
        check_preconditions(p, Or)
        compare_windows(E, Or, "set")
        seen = dict.fromkeys(COUNTS + ("n_jump",), 0)
        for s in range(STEPS):
            re, pe = E.step(S_LIST)
            ro, po = Or.step(S_LIST)
            for k in range(G):
                at = (s, k)
                assert np.array_equal(E.send[k].get(), Or.send[k].get()), at  # all n_send × 416 bytes
                assert re[k] == ro[k], at
                fe, fo = report_fields(pe[k]), report_fields(po[k])
                assert fe == fo, at
                assert fo["n_jump"] <= capi.DD_JCAP and fo["n_xb"] <= capi.DD_XCAP, at  # the lists are whole
                assert jumper_set(*pe[k].jumpers()) == jumper_set(*po[k].jumpers()), at
                assert bond_set(pe[k]) == bond_set(po[k]), at
                for f in seen:
                    seen[f] = max(seen[f], fo[f])
            compare_windows(E, Or, s)
        print(f"resort={resort}: {seen}")
        # the cut was crossed: collisions and a bond between an owned and a halo
        # protein, halo rows that differed (also in a status or link), jumpers
        for f in ("xcol", "xbond", "differed", "n_xb", "links", "n_jump"):
            assert seen[f] > 0, seen
    finally:
        E.close()
        Or.close()


@pytest.fixture(scope="module")
def after():
    """Both families after 20 lockstep steps under KMC_RESORT=3 (read when a
    handle is created), shared by the tests below: each leaves the windows as
    it found them."""
    mp = pytest.MonkeyPatch()
    mp.setenv("KMC_RESORT", "3")
    try:
        p, E, Or = families()
    finally:
        mp.undo()
    check_preconditions(p, Or)
    for _ in range(20):
        E.step(S_LIST)
        Or.step(S_LIST)
    yield p, E, Or
    E.close()
    Or.close()


def test_unpack_crafted_rows(after):
    p, E, Or = after
    k = 2
    me = Or.ranks[k]
    n_a, N = p.n_a, p.n_a + p.n_b
    base = E.received(k)
    assert np.array_equal(base, Or.received(k))
    ids = Or.recv_ids(k)
    band = me.win.band[ids]
    rec = ids < me.win.n_a
    ints = ints_of(base)
    # links that leave the window: proteins of the box this window does not hold
    out_rec = int(np.setdiff1d(np.arange(n_a), me.win.gids)[0])
    out_lig = int(np.setdiff1d(np.arange(n_a, N), me.win.gids)[0])

    def pick(mask, what):
        """A band row and a non-band halo row among the received rows of `mask`."""
        b, h = np.flatnonzero(mask & band), np.flatnonzero(mask & ~band)
        assert b.size and h.size, f"no band / outer-halo row with {what}"
        return int(b[0]), int(h[0])

    def run(first, rows, touched=(), expect=None, where=""):
        reps = [fam.unpack(k, rows, first) for fam in (E, Or)]
        fe, fo = report_fields(reps[0]), report_fields(reps[1])
        # (the oracle lists its jumpers at the finish, the engine at the step: not part of an unpack)
        assert {f: fe[f] for f in COUNTS} == {f: fo[f] for f in COUNTS}, (where, fe, fo)
        if expect is not None:
            assert {f: fe[f] for f in expect} == expect, (where, fe)
        for fam in (E, Or):  # the finish reset the counts
            again = report_fields(fam.ranks[k].eng.dd_finish())
            assert (again["bad"], again["differed"], again["links"], again["n_xb"]) == (0, 0, 0, 0), where
        for i in touched:
            one = ids[i:i + 1]
            assert E.ranks[k].eng.dd_cut_count(one) == Or.ranks[k].eng.dd_cut_count(one), (where, i)
        compare_windows(E, Or, where)
        return E.ranks[k].eng.dd_export(ids)[1]  # the received proteins' ints afterwards

    def restore():
        for fam in (E, Or):
            fam.unpack(k, base, 0)

    try:
        # the unaltered rows are the windows' state: nothing counted
        run(0, base, expect=dict(bad=0, differed=0, links=0), where="unaltered")

        # row counts around the 4 rows of a workgroup and beyond one report's
        # list, from the plan's start and from inside it: the last row differs in
        # a coordinate, the first (when there are two) in a status
        for first in (0, 7):
            for n in (1, 3, 4, 5, 300):
                rows = base[first:first + n].copy()
                set_bead(rows, n - 1, 3, bead_of(rows, n - 1, 3) + 1.0)
                hit = [first + n - 1]
                if n > 1:
                    set_int(rows, 0, 1, 1 - int(ints[first, 1]))
                    hit.append(first)
                run(first, rows, touched=hit, where=f"count {first}+{n}",
                    expect=dict(differed=len(hit), links=n > 1, bad=int(band[hit].sum())))
                restore()

        # a receptor's link to its ligand (nei2) leaves the window: st2, nei2 and nei4 cleared
        for i in pick(rec & (ints[:, 2] > 0), "a receptor–ligand bond"):
            rows = base[i:i + 1].copy()
            set_int(rows, 0, 2, out_lig + 1)
            got = run(i, rows, touched=[i], where=f"nei2 cut, row {i}",
                      expect=dict(differed=1, links=1, bad=int(band[i])))
            assert tuple(got[i, [0, 2, 3]]) == (0, 0, 0) and tuple(got[i, [1, 4]]) == tuple(ints[i, [1, 4]])
            assert E.ranks[k].eng.dd_cut_count(ids[i:i + 1]) == 1
            restore()

        # a receptor's cis link (nei3) leaves the window: st3 and nei3 cleared
        for i in pick(rec & (ints[:, 4] > 0), "a cis bond"):
            rows = base[i:i + 1].copy()
            set_int(rows, 0, 4, out_rec + 1)
            got = run(i, rows, touched=[i], where=f"nei3 cut, row {i}",
                      expect=dict(differed=1, links=1, bad=int(band[i])))
            assert tuple(got[i, [1, 4]]) == (0, 0) and tuple(got[i, [0, 2, 3]]) == tuple(ints[i, [0, 2, 3]])
            assert E.ranks[k].eng.dd_cut_count(ids[i:i + 1]) == 1
            restore()

        # a free ligand's row arrives bound at site j to a receptor outside the
        # window, each site in turn and two at once: cut with its status, so
        # the row equals the window's own (nothing differs), yet the cut is
        # marked and fails the step when the row is in the band
        free = ~rec & (ints[:, :] == 0).all(axis=1)
        for i in pick(free, "a free ligand"):
            for sites in ((1,), (2,), (3,), (4,), (2, 4)):
                rows = base[i:i + 1].copy()
                for j in sites:
                    set_int(rows, 0, j - 1, 1)
                    set_int(rows, 0, 4 + j - 1, out_rec + 1)
                got = run(i, rows, touched=[i], where=f"ligand sites {sites} cut, row {i}",
                          expect=dict(differed=0, links=0, bad=int(band[i])))
                assert not got[i].any()
                assert E.ranks[k].eng.dd_cut_count(ids[i:i + 1]) == 1
                restore()
                assert E.ranks[k].eng.dd_cut_count(ids[i:i + 1]) == 0  # the mark is the last unpack's

        # the same receptor rows bound to a protein the window holds: no cut
        # (a ligand the window holds, by its global index)
        held_lig = int(me.win.gids[me.win.n_a])
        for i in pick(rec & (ints[:, 2] == 0), "a receptor without a ligand"):
            rows = base[i:i + 1].copy()
            set_int(rows, 0, 0, 1)
            set_int(rows, 0, 2, held_lig + 1)
            set_int(rows, 0, 3, 2)
            got = run(i, rows, touched=[i], where=f"held link, row {i}",
                      expect=dict(differed=1, links=1, bad=int(band[i])))
            assert tuple(got[i, [0, 2, 3]]) == (1, me.win.n_a + 1, 2)
            assert E.ranks[k].eng.dd_cut_count(ids[i:i + 1]) == 0
            restore()

        # the compare is bitwise: +0.0 against -0.0 differs
        for i in pick(rec, "a receptor"):
            rows = base[i:i + 1].copy()
            set_bead(rows, 0, 5, 0.0)  # (a membrane receptor's z may be +0.0 already)
            run(i, rows, where=f"zero, row {i}")
            set_bead(rows, 0, 5, -0.0)
            run(i, rows, where=f"sign of zero, row {i}", expect=dict(differed=1, links=0, bad=int(band[i])))
            run(i, rows, where=f"sign of zero again, row {i}", expect=dict(differed=0, links=0, bad=0))
            restore()

        # a status alone differs: counted as a link difference
        for i in pick(rec & (ints[:, 4] == 0), "a receptor without a cis bond"):
            rows = base[i:i + 1].copy()
            set_int(rows, 0, 1, 1)
            got = run(i, rows, touched=[i], where=f"status, row {i}",
                      expect=dict(differed=1, links=1, bad=int(band[i])))
            assert got[i, 1] == 1
            restore()
    finally:
        restore()
        for fam in (E, Or):
            fam.ranks[k].eng.dd_finish()
    compare_windows(E, Or, "restored")


def test_import_flags(after):
    p, E, Or = after
    k = 1
    me = Or.ranks[k]
    n_a = me.win.n_a
    halo = Or.recv_ids(k)
    hr, hl = halo[halo < n_a], halo[halo >= n_a]
    assert hr.size >= 4 and hl.size >= 4
    sel = np.array([hr[0], hl[0], hr[1], hr[2], hl[1], hl[2], hr[3], hl[3]], dtype=np.int32)
    other = int(hr[5])  # a held receptor (local index) for the altered links
    beads0, ints0 = Or.ranks[k].eng.dd_export(sel)
    assert same_export((beads0, ints0), E.ranks[k].eng.dd_export(sel))
    try:
        for n in (1, 2, 3, 5, 8):
            for shift in range(4):
                # kinds in turn over neighbouring ids, which share a 32-bit word of flags:
                # 1 a coordinate, 2 a status and its link, 3 both, 0 nothing
                kinds = [(i + shift + 1) % 4 for i in range(n)]
                beads, ints = beads0[:n].copy(), ints0[:n].copy()
                for i, kind in enumerate(kinds):
                    receptor = sel[i] < n_a
                    if kind & 1:
                        e = (7 * i + shift) % (48 if receptor else 24)
                        beads[i, e] = np.nextafter(beads[i, e], np.inf)
                    if kind & 2:
                        st, lk = (1, 4) if receptor else (2, 6)  # cis link / site 3
                        assert ints[i, lk] != other + 1
                        ints[i, st], ints[i, lk] = 1, other + 1
                fe = E.ranks[k].eng.dd_import(sel[:n], beads, ints)
                fo = Or.ranks[k].eng.dd_import(sel[:n], beads, ints)
                assert fe.tolist() == fo.tolist() == kinds, (n, shift)
                assert same_export(E.export_all(k), Or.export_all(k)), (n, shift)
                got = E.ranks[k].eng.dd_export(sel[:n])
                assert same_export(got, (beads, ints)), (n, shift)
                # importing the same again: nothing differs
                assert not E.ranks[k].eng.dd_import(sel[:n], beads, ints).any()
                assert not Or.ranks[k].eng.dd_import(sel[:n], beads, ints).any()
                for fam in (E, Or):
                    fam.ranks[k].eng.dd_import(sel[:n], beads0[:n], ints0[:n])
    finally:
        for fam in (E, Or):
            fam.ranks[k].eng.dd_import(sel, beads0, ints0)
    compare_windows(E, Or, "restored")


def test_jumpers_and_drift(after):
    p, E, Or = after
    L = p.box_x
    crossed = 0
    for k in range(G):
        e, o = E.ranks[k].eng, Or.ranks[k].eng
        own = np.flatnonzero(Or.ranks[k].win.own).astype(np.int32)
        x = o.dd_export(own)[0][:, 0]
        raw = x - Or.x0[k][own]
        d = np.abs(raw - L * np.round(raw / L))  # the periodic displacement, as the kernels compute it
        seam = np.flatnonzero(np.abs(raw) > L / 2)  # crossed the periodic seam since the windows were set
        crossed += seam.size
        t = int(seam[0]) if seam.size else int(np.argsort(d)[d.size // 2])
        assert 0.0 < d[t] < d.max() and (not seam.size or d[t] < 200.0)
        assert e.dd_drift() == o.dd_drift() == float(np.float32(d.max()))
        below = float(np.nextafter(d[t], 0.0))
        sizes = {}
        for S in (0.0, float(d[t]), below, float(d.max()) + 1.0):
            je, jo = jumper_set(*e.dd_jumpers(S)), jumper_set(*o.dd_jumpers(S))
            assert je == jo, (k, S)
            assert jo == jumper_set(own[d > S], x[d > S]), (k, S)
            sizes[S] = len(jo)
        # strictly more than S: the protein displaced by exactly S is not listed, just below S it is
        assert int(own[t]) not in o.dd_jumpers(float(d[t]))[0] and int(own[t]) in o.dd_jumpers(below)[0]
        assert sizes[below] == sizes[float(d[t])] + int((d == d[t]).sum())
        assert sizes[0.0] > capi.DD_JCAP and sizes[float(d.max()) + 1.0] == 0
        full = jumper_set(*o.dd_jumpers(0.0))
        for cap in (5, 0):  # fewer than there are: *n is the whole count, the entries some of them
            n, ids, xs = raw_jumpers(e, 0.0, cap)
            got = jumper_set(ids, xs)
            assert n == len(full) and len(got) == cap and got <= full, (k, cap)
    assert crossed > 0, "no owned protein crossed the x seam since the windows were set"

    # a step that lists more than the report holds: the count is whole, the
    # KMC_DD_JCAP entries are distinct members of the whole list
    re, pe = E.step(0.0)
    ro, po = Or.step(0.0)
    for k in range(G):
        assert re[k] == ro[k] and np.array_equal(E.send[k].get(), Or.send[k].get())
        fe, fo = report_fields(pe[k]), report_fields(po[k])
        assert fe == fo and fo["n_jump"] > capi.DD_JCAP, (k, fe, fo)
        full = jumper_set(*Or.ranks[k].eng.dd_jumpers(0.0))
        assert len(full) == fo["n_jump"]
        got = jumper_set(*pe[k].jumpers())
        assert len(got) == capi.DD_JCAP and got <= full, k
    compare_windows(E, Or, "after the step")

