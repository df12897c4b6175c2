"""tests/golden/big_complexes.npz (make_big_complexes.py) holds what the GPU
tests of test_gpu_complex_sizes.py rely on — no GPU: the component sizes of
every stored state, recomputed by a plain union-find over the link arrays, at
both sides of the step engine's switches (CXL = 16 members: streamed / global
-memory path, with moves that are committed; BFS_QCAP = 32: LDS queue /
overflow list; above 64), a ring in
the bond graph, valid states, and S16's next 50 oracle steps against the stored
hashes."""
import numpy as np
import pytest

import _complex as CX
from _kmc import O, capi, engine
from _rings import ref_rings


@pytest.fixture(scope="module")
def states():
    return {name: CX.load(name) for name in CX.names()}


def test_states_are_valid(states):
    assert set(states) == {"S16", "S17", "S32", "S64"}
    for name, (p, hs) in states.items():
        assert engine.host_validate(p, hs) == capi.KMC_OK, name


def test_s16_sizes(states):
    s = CX.sizes(states["S16"][1])
    assert 15 in s and CX.CXL in s and s[0] >= CX.CXL + 1, s


def test_s17_sizes_and_committed_moves(states):
    # S16 is jammed: its complexes of 15, 16 and 17 members collide on every step.  S17 holds the same sizes, each
    # rejected on some steps and accepted on the others (the oracle's collision tests by member count)
    p, hs = states["S17"]
    assert CX.sizes(hs) == [17, 16, 15]
    for name, committed in (("S16", False), ("S17", True)):
        p, hs = states[name]
        o = O.Oracle(p, rng_mode=O.RNG_KEYED, nbmode=O.NB_CELLS)
        o.set_state(hs)
        o.step(200, want_hashes=False)
        rej, acc = o.complex_outcomes()
        assert rej[15:18].min() > 0 and (acc[15:18].min() > 0) == committed and (acc[15:18].max() > 0) == committed, name


def test_s32_sizes(states):
    hs = states["S32"][1]
    s = CX.sizes(hs)
    assert s.count(CX.BFS_QCAP) == 1 and s[0] >= CX.BFS_QCAP + 1, s
    assert CX.ligands_of_largest(hs) >= 2  # entered by the BFS from a ligand that is not its root
    assert CX.expected_overflow(hs) >= 1


def test_s64_sizes(states):
    hs = states["S64"][1]
    assert CX.sizes(hs)[0] > 64
    assert CX.expected_overflow(hs) >= 2  # a ligand other than the root reaches the overflow BFS too


def test_a_ring_in_the_bond_graph(states):
    for name in ("S32", "S64"):
        counts, member = ref_rings(states[name][1], 6)
        assert counts[0, 6] == 1 and int(np.count_nonzero(member[0])) == 6, name


def test_s16_replays_the_stored_hashes(states):
    p, hs = states["S16"]
    o = O.Oracle(p, rng_mode=O.RNG_KEYED, nbmode=O.NB_CELLS)
    o.set_state(hs)
    assert engine.state_hash(p, o.get_state()) == o.hash()
    _, hashes = o.step(50)
    assert np.array_equal(hashes, CX.stored("S16_hashes50"))
