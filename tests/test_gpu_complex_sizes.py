"""The step engine where the size of a complex switches its code path
(DESIGN.md §3a), from the CPU-made states of tests/golden/big_complexes.npz:

  S16  complexes of 15, 16 and 17 members at once — CXL = 16 is the last size
       with member records (mrec) on the streamed / LDS-staged path, 17 the
       first on the global-memory path of k_complex_heavy; 15 and 17 leave
       ragged last batches in cx_params, register_complex and the BFS.  The
       state is jammed: the complexes of 15, 16 and 17 members collide on every
       step (the rejection's row copy of a large unit) and none of their moves
       is ever committed — here the comparison checks the unit rows, the
       decision to reject and the restored state.
  S17  three hand-linked rings of four ligands with 15, 16 and 17 members, each
       rejected on some steps and accepted with changed beads on the others:
       the beads and records of the staged path at its full width and of the
       global-memory path at its first size, committed.
  S32  a component of exactly 32 members, the last that fits bfs_one's queue,
       and one of 33, the first on the overflow list (bfs_overflow_one inside
       k_complex_heavy), with nine ligands that enter it and a ring of six.
       Neither is ever rejected; the 32 is at rest and passes through the
       global-memory path unchanged, the 33 is re-aligned, changed and
       committed on every step.
  S64  a component of 72 members and 24 ligands; three of them reach the
       overflow BFS, two of which are not its root.  Changed and committed on
       every step.

Every case steps the engine one step at a time from the fixture state beside
the keyed oracle started from the same state: every bond.dat record and the
full-state hash after every step are equal, in the cases that say so also every
unit row of kmc_get_clusters (rows and member order).  Before it compares, a
case asserts from the state (a plain union-find, _complex.py) the sizes it is
there for; the oracle's event counts, its collision tests by complex size
(Oracle.complex_outcomes), the complexes whose beads changed between its
consecutive states, and the sizes after the window are asserted once, where the
window is computed."""
import re

import pytest

import _complex as CX
from _kmc import O, compare_stepwise, engine, stats_delta
from _scale import FAST

pytestmark = pytest.mark.gpu

STEPS = 200
# test_large_complex_breaks_and_merges: the dense association rates, every dissociation rate at FAST
FAST_KW = dict(ass_rate=0.09, cis_ass_rate=0.09, mono_cis_ass_rate=0.01, diss_rate=FAST, cis_diss_rate=FAST,
               mono_cis_diss_rate=FAST)


class Window:
    """STEPS oracle steps from a fixture state, computed once, shared and left unchanged."""

    def __init__(self, name, **overrides):
        self.p, self.st = CX.load(name, **overrides)
        o = O.Oracle(self.p, rng_mode=O.RNG_KEYED, nbmode=O.NB_CELLS)
        o.set_state(self.st)
        s0 = o.stats()
        self.obs, self.hashes, self.rows, self.breaks, self.merges = [], [], [], {}, {}
        self.changed = {}  # member count -> complex-steps in which a bead of a complex of that size changed
        prev = self.st
        for _ in range(STEPS):
            rec, h = o.step(1)
            self.obs.append(rec[0])
            self.hashes.append(int(h[0]))
            self.rows.append(CX.unit_rows(*o.clusters()))
            cur = o.get_state()
            for n in CX.changed_sizes(prev, cur):
                self.changed[n] = self.changed.get(n, 0) + 1
            if overrides:
                for limit in (CX.CXL, CX.BFS_QCAP):
                    b, m = CX.break_and_merge(prev, cur, limit)
                    self.breaks[limit] = self.breaks.get(limit, 0) + b
                    self.merges[limit] = self.merges.get(limit, 0) + m
            prev = cur
        self.events = stats_delta(s0, o.stats())
        # the complexes' collision tests by member count (the events' reject count includes the free units)
        self.rejected, self.accepted = o.complex_outcomes()
        self.sizes0, self.sizes1 = CX.sizes(self.st), CX.sizes(cur)
        self.run = (self.obs, self.hashes)


def _complex_work(w):
    """What every window must hold: complex moves, multi-ligand alignments with a repeat pass, rejections."""
    e = w.events
    assert e["complex"] >= STEPS and e["multi"] >= STEPS and e["repeat"] > 0 and e["reject"] > 0, e


@pytest.fixture(scope="module")
def s16():
    w = Window("S16")
    s = w.sizes0
    assert 15 in s and CX.CXL in s and s.count(CX.CXL + 1) == 2, s
    _complex_work(w)
    # no rate can change a size: 17 complexes a step, both paths on every compared step
    assert w.sizes1 == s and w.events["complex"] == STEPS * len(s) and w.events["laydown"] > 0, (w.sizes1, w.events)
    # the jam: both complexes of 17 collide on every step, as do the 16 and the 15 (of the 3400 complex moves of
    # this window 3200 are rejected, one complex of 11 is accepted unchanged on every step; 219 more rejections are
    # free units): the rejection of a large unit on every step, and no committed move at these sizes — S17's part
    for n, k in ((17, 2), (16, 1), (15, 1)):
        assert w.rejected[n] == k * STEPS and w.accepted[n] == 0, (n, w.rejected[n], w.accepted[n])
    assert not w.changed, w.changed
    return w


@pytest.fixture(scope="module")
def s17():
    w = Window("S17")
    assert w.sizes0 == [17, 16, 15] and w.sizes1 == w.sizes0, (w.sizes0, w.sizes1)
    _complex_work(w)
    # each of the three is rejected on some steps and accepted on others, and a bead of it differs after every
    # accepted move (this window: 15 members 79 / 121, 16 78 / 122, 17 176 / 24): the staged path at its full width
    # and the global-memory path at its first size are compared on moves that were committed
    for n in (15, 16, 17):
        assert w.rejected[n] > 0 and w.accepted[n] > 0 and w.rejected[n] + w.accepted[n] == STEPS, n
        assert w.changed.get(n, 0) == w.accepted[n], (n, w.changed, w.accepted[n])
    return w


@pytest.fixture(scope="module")
def s32():
    w = Window("S32")
    s = w.sizes0
    assert s.count(CX.BFS_QCAP) == 1 and s[0] == CX.BFS_QCAP + 1 and CX.ligands_of_largest(w.st) >= 2, s
    assert CX.expected_overflow(w.st) == 1
    _complex_work(w)
    assert w.sizes1 == s, w.sizes1
    # neither is ever rejected (this window's 17 rejections are free units).  The chain of 32 is at rest: the
    # global-memory path passes it through unchanged on every step.  The 33 is re-aligned, changed and committed
    # on every step; all snaps of the window are its own
    assert w.accepted[32] == w.accepted[33] == STEPS and w.rejected[32] == w.rejected[33] == 0
    assert w.changed.get(33, 0) == STEPS and w.changed.get(32, 0) == 0, w.changed
    assert w.events["snap_bond"] > STEPS and w.events["snap_cis"] > STEPS, w.events
    return w


@pytest.fixture(scope="module")
def s64():
    w = Window("S64")
    assert w.sizes0[0] > 64 and CX.ligands_of_largest(w.st) >= 2, w.sizes0
    assert CX.expected_overflow(w.st) == 3
    _complex_work(w)
    # the 72 is never rejected (the 85 rejections are free units): changed and committed on every step
    assert w.sizes1 == w.sizes0 and w.accepted[72] == STEPS and w.changed.get(72, 0) == STEPS, (w.sizes1, w.changed)
    return w


@pytest.fixture(scope="module")
def windows(s16, s17, s32):
    return {"S16": s16, "S17": s17, "S32": s32}


def _stepwise(w, steps=STEPS, rows=True, start=None, first=0):
    """The engine from w's state (or `start`, the state after `first` steps), one step at a time: records, hashes
    and, with rows, the unit rows equal w's."""
    with engine.Simulation(w.p) as sim:
        sim.set_state(w.st if start is None else start)
        for s in range(first, steps):
            rec = sim.step(1)
            assert rec[0] == w.obs[s], f"step {s + 1}: record {rec[0]} != {w.obs[s]}"
            hs = sim.get_state()
            h = engine.state_hash(w.p, hs)
            assert h == w.hashes[s], f"step {s + 1}: hash {h:x} != {w.hashes[s]:x}"
            if rows:
                got = CX.unit_rows(*sim.clusters())
                assert got == w.rows[s], f"step {s + 1}: unit rows differ from the oracle's"
    return hs


def _overflow_counts(err):
    return [int(x) for x in re.findall(r"bfs-overflow (\d+)", err)]


def test_sizes_15_16_17(s16):
    _stepwise(s16)


def test_accepted_15_16_17(s17):
    _stepwise(s17)


def test_queue_full_and_overflow(monkeypatch, capfd, s32):
    monkeypatch.setenv("KMC_DEBUG_COUNTS", "1")
    _stepwise(s32)
    n = _overflow_counts(capfd.readouterr().err)
    # the first step rebuilds every complex: the root of the 33 is the one ligand on the overflow list (the other
    # eight see a lower ligand among their first 32 members and give up before the append); the complex is kept
    # from step to step, and every later full rebuild (a re-sort) lists the same one
    assert len(n) == STEPS and n[0] == CX.expected_overflow(s32.st) and set(n) <= {0, n[0]}, n[:5]


def test_above_64(monkeypatch, capfd, s64):
    monkeypatch.setenv("KMC_DEBUG_COUNTS", "1")
    _stepwise(s64)
    n = _overflow_counts(capfd.readouterr().err)
    assert len(n) == STEPS and n[0] == CX.expected_overflow(s64.st) and set(n) <= {0, n[0]}, n[:5]


# one axis at a time against the default: the stand-alone k_bfs, the side-stream modes (which also run it), no
# re-sort and one every seven steps (the slots renumbered under a kept descriptor, the members[] cursor reset)
ARRANGEMENTS = [("KMC_STEP_CHAIN", "0"), ("KMC_CX_STREAM", "0"), ("KMC_CX_STREAM", "1"), ("KMC_CX_STREAM", "2"),
                ("KMC_CX_STREAM", "3"), ("KMC_RESORT", "0"), ("KMC_RESORT", "7")]


@pytest.mark.parametrize("knob,value", ARRANGEMENTS)
@pytest.mark.parametrize("name", ["S16", "S17", "S32"])
def test_arrangements(monkeypatch, windows, name, knob, value):
    monkeypatch.setenv(knob, value)
    w = windows[name]
    compare_stepwise(w.p, STEPS, nbmode=O.NB_CELLS, init_state=w.st, oracle_run=w.run)


@pytest.fixture(scope="module")
def fast():
    """S16 and S32 continued at the raised dissociation rates: complexes above 16 (32) members lose bonds and fall
    to pieces below, smaller ones merge past the limit (this build, 200 steps: S16 8 breaks and 6 merges across
    16 | 17; S32 3 and 2, and 1 break across 32 | 33)."""
    out = {name: Window(name, **FAST_KW) for name in ("S16", "S32")}
    for name, w in out.items():
        assert w.breaks[CX.CXL] > 0 and w.merges[CX.CXL] > 0, (name, w.breaks, w.merges)
        assert w.events["rld"] > 0 and w.events["cd"] > 0 and w.events["rl"] > 0, (name, w.events)
    assert out["S32"].breaks[CX.BFS_QCAP] > 0, out["S32"].breaks
    return out


@pytest.mark.parametrize("name", ["S16", "S32"])
def test_large_complex_breaks_and_merges(fast, name):
    _stepwise(fast[name])


def test_poisoned_rnew_with_large_complexes(monkeypatch, s32):
    # R_new poisoned before every step and every record's step checked: a member bead or record the global-memory
    # path forgets to write is a mismatch or a latched error
    monkeypatch.setenv("KMC_DEBUG_POISON", "1")
    monkeypatch.setenv("KMC_DEBUG_RECS", "1")
    _stepwise(s32, rows=False)


@pytest.mark.parametrize("name", ["S16", "S17", "S32"])
def test_exact_resume_with_large_complexes(windows, name):
    # the descriptors are rebuilt from the links alone: a state taken after 100 steps and continued in a new
    # handle ends where the uninterrupted oracle does
    w = windows[name]
    mid = _stepwise(w, steps=100, rows=False)
    _stepwise(w, rows=True, start=mid, first=100)
